// Stand-alone check of the host-side merges of the shards' report rows
// (go-libp2p-pubsub_amd/csrc/report_merge.cpp), meant for the host sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Igo-libp2p-pubsub_amd/csrc tools/report_merge_check.cpp \
//       go-libp2p-pubsub_amd/csrc/report_merge.cpp -o report_merge_check && ./report_merge_check
//
// One section per merge: msg, net, peer, score, mesh_paths, relay.  An argument
// runs that section alone, no argument runs all six.  Exit status 0 and the
// section's "... merge ok" line when every case of it holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "report_merge.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static const double kInf = std::numeric_limits<double>::infinity();

// ---- the propagation report: merge_reports ----
namespace msg_check {

using Row = struct gsim_msg_report;

static Row row(uint32_t slot, uint64_t id, int64_t pub, uint32_t topic, uint32_t origin)
{
    Row r;
    std::memset(&r, 0, sizeof r);
    r.slot = slot; r.id = id; r.pub_round = pub; r.topic = topic; r.origin = origin;
    return r;
}

static void add(Row& r, int bin, uint32_t n, uint32_t exact)
{
    r.hist[bin] += n;
    r.reached += n;
    if (exact > r.max_latency) r.max_latency = exact;
}

static int merge(const std::vector<std::vector<Row>>& parts, const std::vector<std::vector<uint32_t>>& gid,
                 std::vector<Row>* out)
{
    std::vector<const Row*> pp;
    std::vector<const uint32_t*> gp;
    std::vector<size_t> gn;
    for (size_t l = 0; l < parts.size(); ++l) {
        pp.push_back(parts[l].data());
        gp.push_back(gid[l].data());
        gn.push_back(gid[l].size());
    }
    const size_t rows = parts.empty() ? 0 : parts[0].size();
    out->assign(rows, Row{});
    return gsim::merge_reports(pp.data(), gp.data(), gn.data(), pp.size(), rows, out->data());
}

static int run()
{
    static_assert(sizeof(Row) == 176, "struct gsim_msg_report is 176 bytes");
    const uint32_t none = 0xFFFFFFFFu;
    // three shards over 9 peers: local ids (owned + ghosts) -> global ids
    const std::vector<std::vector<uint32_t>> gid = {{0, 1, 2, 5}, {1, 3, 4, 5, 8}, {2, 6, 7, 8}};
    std::vector<std::vector<Row>> parts(3);
    // slot 4: origin global 5, a ghost on shards 0 and 1, unknown to shard 2
    parts[0].push_back(row(4, 100, 12, 1, 3));
    parts[1].push_back(row(4, 100, 12, 1, 3));
    parts[2].push_back(row(4, 100, 12, 1, none));
    add(parts[0][0], 0, 0, 0); add(parts[0][0], 1, 2, 1); parts[0][0].subscribers = 3;
    add(parts[1][0], 0, 1, 0); add(parts[1][0], 2, 1, 2); parts[1][0].subscribers = 2;
    add(parts[2][0], 31, 3, 40); parts[2][0].subscribers = 4;
    // slot 7: origin global 8, known only to the last shard
    parts[0].push_back(row(7, 101, 13, 0, none));
    parts[1].push_back(row(7, 101, 13, 0, 4));
    parts[2].push_back(row(7, 101, 13, 0, 3));
    add(parts[2][1], 0, 1, 0); parts[2][1].subscribers = 1;
    std::vector<Row> out;
    CHECK(merge(parts, gid, &out) == GSIM_OK);
    CHECK(out.size() == 2);
    CHECK(out[0].origin == 5 && out[0].slot == 4 && out[0].id == 100 && out[0].pub_round == 12 && out[0].topic == 1);
    CHECK(out[0].hist[0] == 1 && out[0].hist[1] == 2 && out[0].hist[2] == 1 && out[0].hist[31] == 3);
    CHECK(out[0].reached == 7 && out[0].subscribers == 9 && out[0].max_latency == 40);
    CHECK(out[1].origin == 8 && out[1].reached == 1 && out[1].subscribers == 1 && out[1].max_latency == 0);
    uint32_t sum = 0;
    for (int q = 0; q < GSIM_REPORT_BINS; ++q) sum += out[0].hist[q];
    CHECK(sum == out[0].reached);
    // one shard: the rows in global ids; no origin known anywhere stays 0xFFFFFFFF
    std::vector<std::vector<Row>> one = {{parts[0][1]}};
    CHECK(merge(one, {gid[0]}, &out) == GSIM_OK && out.size() == 1 && out[0].origin == none);
    // no rows, no parts
    const std::vector<std::vector<Row>> empty2(2), empty0;
    CHECK(merge(empty2, {gid[0], gid[1]}, &out) == GSIM_OK && out.empty());
    CHECK(merge(empty0, {}, &out) == GSIM_OK && out.empty());
    // disagreements: another message in the slot, another origin, an origin outside the id table
    auto bad = parts;
    bad[1][0].id = 999;
    CHECK(merge(bad, gid, &out) == GSIM_ESTATE);
    bad = parts;
    bad[1][0].pub_round = 11;
    CHECK(merge(bad, gid, &out) == GSIM_ESTATE);
    bad = parts;
    bad[1][0].origin = 0;                      // global 1, not 5
    CHECK(merge(bad, gid, &out) == GSIM_ESTATE);
    bad = parts;
    bad[2][1].origin = 4;                      // shard 2 has local ids 0..3 only
    CHECK(merge(bad, gid, &out) == GSIM_ESTATE);
    bad = parts;
    bad[0][0].origin = 4;
    CHECK(merge(bad, gid, &out) == GSIM_ESTATE);
    if (!fails) std::printf("report merge ok\n");
    return fails ? 1 : 0;
}

}  // namespace msg_check

// ---- the network report: merge_net_reports ----
namespace net_check {

using Mesh = struct gsim_mesh_row;
using Score = struct gsim_score_row;

static Mesh mesh_row(uint32_t topic, uint32_t cls)
{
    Mesh r;
    std::memset(&r, 0, sizeof r);
    r.topic = topic; r.cls = cls;
    return r;
}

// a member with mesh size d, o of it outbound, every link into class `into`
static void member(Mesh& r, uint32_t d, uint32_t o, int into)
{
    r.members += 1;
    r.deg_hist[d < GSIM_NET_DEG_BINS - 1 ? d : GSIM_NET_DEG_BINS - 1] += 1;
    r.out_hist[o < GSIM_NET_OUT_BINS - 1 ? o : GSIM_NET_OUT_BINS - 1] += 1;
    r.mesh_links[into] += d;
    r.outbound_links += o;
    if (d > r.max_degree) r.max_degree = d;
}

static Score score_row(uint32_t a, uint32_t b)
{
    Score r;
    std::memset(&r, 0, sizeof r);
    r.obs_cls = a; r.subj_cls = b;
    r.min = kInf; r.max = -kInf;
    return r;
}

static void score(Score& r, int bin, double s)
{
    r.connected += 1;
    r.hist[bin] += 1;
    if (s < r.min) r.min = s;
    if (s > r.max) r.max = s;
}

static int merge(const std::vector<std::vector<Mesh>>& mp, const std::vector<std::vector<Score>>& sp,
                 std::vector<Mesh>* mo, std::vector<Score>* so)
{
    std::vector<const Mesh*> mpp;
    std::vector<const Score*> spp;
    for (auto& p : mp) mpp.push_back(p.data());
    for (auto& p : sp) spp.push_back(p.data());
    const size_t L = mp.empty() ? sp.size() : mp.size();
    const size_t nm = mp.empty() ? 0 : mp[0].size(), ns = sp.empty() ? 0 : sp[0].size();
    mo->assign(nm, Mesh{});
    so->assign(ns, Score{});
    return gsim::merge_net_reports(mp.empty() ? nullptr : mpp.data(), sp.empty() ? nullptr : spp.data(), L, nm, ns,
                                   mp.empty() ? nullptr : mo->data(), sp.empty() ? nullptr : so->data());
}

static int run()
{
    // three shards, two topics x two classes, two class pairs shown of four
    std::vector<std::vector<Mesh>> mp(3);
    std::vector<std::vector<Score>> sp(3);
    for (int l = 0; l < 3; ++l) {
        for (uint32_t t = 0; t < 2; ++t)
            for (uint32_t c = 0; c < 2; ++c) mp[l].push_back(mesh_row(t, c));
        for (uint32_t a = 0; a < 2; ++a)
            for (uint32_t b = 0; b < 2; ++b) sp[l].push_back(score_row(a, b));
    }
    member(mp[0][0], 8, 2, 0);
    member(mp[0][0], 40, 9, 1);         // the overflow bins; the largest mesh
    member(mp[1][0], 6, 0, 1);
    member(mp[2][0], 33, 7, 0);
    member(mp[2][3], 5, 1, 1);
    mp[1][1].fanout_peers = 2; mp[1][1].fanout_links = 11;
    mp[2][1].fanout_peers = 1; mp[2][1].fanout_links = 6;
    score(sp[0][0], 3, -1.5);
    score(sp[1][0], 0, -kInf);
    score(sp[2][0], 15, 7.25);
    sp[1][0].nan = 2; sp[1][0].connected += 2;
    sp[2][0].retained = 5;
    score(sp[1][3], 2, -0.0);            // the only part with an edge of pair (1, 1)
    std::vector<Mesh> mo;
    std::vector<Score> so;
    CHECK(merge(mp, sp, &mo, &so) == GSIM_OK);
    CHECK(mo.size() == 4 && so.size() == 4);
    CHECK(mo[0].topic == 0 && mo[0].cls == 0 && mo[3].topic == 1 && mo[3].cls == 1);
    CHECK(mo[0].members == 4 && mo[0].max_degree == 40);
    CHECK(mo[0].deg_hist[8] == 1 && mo[0].deg_hist[6] == 1 && mo[0].deg_hist[31] == 2);
    CHECK(mo[0].out_hist[2] == 1 && mo[0].out_hist[0] == 1 && mo[0].out_hist[7] == 2);
    CHECK(mo[0].mesh_links[0] == 41 && mo[0].mesh_links[1] == 46 && mo[0].mesh_links[2] == 0);
    CHECK(mo[0].outbound_links == 18);
    CHECK(mo[1].members == 0 && mo[1].fanout_peers == 3 && mo[1].fanout_links == 17 && mo[1].max_degree == 0);
    CHECK(mo[2].members == 0 && mo[2].max_degree == 0);
    CHECK(mo[3].members == 1 && mo[3].deg_hist[5] == 1 && mo[3].mesh_links[1] == 5 && mo[3].max_degree == 5);
    uint32_t sd = 0, sout = 0;
    for (int q = 0; q < GSIM_NET_DEG_BINS; ++q) sd += mo[0].deg_hist[q];
    for (int q = 0; q < GSIM_NET_OUT_BINS; ++q) sout += mo[0].out_hist[q];
    CHECK(sd == mo[0].members && sout == mo[0].members);
    CHECK(so[0].connected == 5 && so[0].nan == 2 && so[0].retained == 5);
    CHECK(so[0].hist[0] == 1 && so[0].hist[3] == 1 && so[0].hist[15] == 1);
    CHECK(so[0].min == -kInf && so[0].max == 7.25);
    // a pair nobody has an edge of keeps the identities
    CHECK(so[1].connected == 0 && so[1].min == kInf && so[1].max == -kInf);
    CHECK(so[2].connected == 0 && so[2].min == kInf && so[2].max == -kInf);
    // a pair only one part has: that part's min and max (the identities of the others change nothing)
    CHECK(so[3].connected == 1 && so[3].min == 0.0 && so[3].max == 0.0 && std::signbit(so[3].min));

    // one part: a copy
    {
        std::vector<std::vector<Mesh>> m1(1, mp[0]);
        std::vector<std::vector<Score>> s1(1, sp[0]);
        CHECK(merge(m1, s1, &mo, &so) == GSIM_OK);
        CHECK(std::memcmp(mo.data(), mp[0].data(), sizeof(Mesh) * 4) == 0);
        CHECK(std::memcmp(so.data(), sp[0].data(), sizeof(Score) * 4) == 0);
    }
    // either half alone; no rows at all
    {
        std::vector<std::vector<Mesh>> none_m;
        std::vector<std::vector<Score>> none_s;
        CHECK(merge(mp, none_s, &mo, &so) == GSIM_OK && mo[0].members == 4 && so.empty());
        CHECK(merge(none_m, sp, &mo, &so) == GSIM_OK && so[0].connected == 5 && mo.empty());
        std::vector<std::vector<Mesh>> em(2);
        std::vector<std::vector<Score>> es(2);
        CHECK(merge(em, es, &mo, &so) == GSIM_OK);
    }
    // disagreements about a row's key are refused
    {
        auto bad = mp;
        bad[1][2].cls = 1;
        CHECK(merge(bad, sp, &mo, &so) == GSIM_ESTATE);
        bad = mp;
        bad[2][1].topic = 1;
        CHECK(merge(bad, sp, &mo, &so) == GSIM_ESTATE);
        auto sbad = sp;
        sbad[2][1].subj_cls = 0;
        CHECK(merge(mp, sbad, &mo, &so) == GSIM_ESTATE);
        sbad = sp;
        sbad[1][3].obs_cls = 0;
        CHECK(merge(mp, sbad, &mo, &so) == GSIM_ESTATE);
    }
    if (fails) return 1;
    std::printf("net report merge ok\n");
    return 0;
}

}  // namespace net_check

// ---- the peer delivery report: merge_peer_reports ----
namespace peer_check {

using Row = struct gsim_peer_class_row;

static Row row(uint32_t topic, uint32_t cls, uint32_t peers, uint32_t messages)
{
    Row r;
    std::memset(&r, 0, sizeof r);
    r.topic = topic; r.cls = cls; r.peers = peers; r.messages = messages;
    r.expected = (uint64_t)peers * messages;
    r.missed = r.expected;
    return r;
}

// one delivery at latency d from a sender of class `from` (from < 0: the peer's own publication)
static void delivery(Row& r, uint32_t d, int from)
{
    r.received += 1;
    r.missed -= 1;
    r.hist[d < GSIM_REPORT_BINS - 1 ? d : GSIM_REPORT_BINS - 1] += 1;
    r.lat_sum += d;
    if (d > r.lat_max) r.lat_max = d;
    if (from < 0) r.own += 1; else r.first_from[from] += 1;
}

static int merge(const std::vector<std::vector<Row>>& parts, const std::vector<int64_t>& nm, std::vector<Row>* out)
{
    std::vector<const Row*> pp;
    for (auto& p : parts) pp.push_back(p.data());
    const size_t rows = parts.empty() ? 0 : parts[0].size();
    out->assign(rows, Row{});
    return gsim::merge_peer_reports(pp.data(), nm.data(), parts.size(), rows, out->data());
}

static int run()
{
    CHECK(sizeof(Row) == 352 && sizeof(struct gsim_peer_row) == 48);
    // three shards, two topics x two classes; topic 0 has 5 selected messages, topic 1 has 3
    std::vector<std::vector<Row>> parts(3);
    const uint32_t peers[3][4] = {{10, 2, 7, 0}, {20, 0, 7, 1}, {30, 1, 0, 0}};
    for (int l = 0; l < 3; ++l)
        for (uint32_t t = 0; t < 2; ++t)
            for (uint32_t c = 0; c < 2; ++c) parts[l].push_back(row(t, c, peers[l][t * 2 + c], t == 0 ? 5 : 3));
    std::vector<int64_t> nm(3, 8);
    delivery(parts[0][0], 0, -1);
    delivery(parts[0][0], 2, 0);
    delivery(parts[0][0], 40, 1);          // the overflow bin; the largest latency
    delivery(parts[1][0], 3, 1);
    delivery(parts[2][0], 33, 0);
    delivery(parts[1][3], 1, 0);           // the only part with a delivery in row (1, 1)
    parts[2][1].received = 2; parts[2][1].hist[4] = 2; parts[2][1].lat_sum = 8; parts[2][1].lat_max = 4;
    parts[2][1].first_from[1] = 2;         // strays: received by peers that do not announce: missed stays
    std::vector<Row> out;
    CHECK(merge(parts, nm, &out) == GSIM_OK);
    CHECK(out.size() == 4);
    CHECK(out[0].topic == 0 && out[0].cls == 0 && out[3].topic == 1 && out[3].cls == 1);
    CHECK(out[0].peers == 60 && out[0].messages == 5 && out[0].expected == 300);
    CHECK(out[0].received == 5 && out[0].own == 1 && out[0].missed == 295);
    CHECK(out[0].lat_sum == 78 && out[0].lat_max == 40);
    CHECK(out[0].hist[0] == 1 && out[0].hist[2] == 1 && out[0].hist[3] == 1 && out[0].hist[31] == 2);
    CHECK(out[0].first_from[0] == 2 && out[0].first_from[1] == 2 && out[0].first_from[2] == 0);
    uint64_t sh = 0, sf = 0;
    for (int q = 0; q < GSIM_REPORT_BINS; ++q) sh += out[0].hist[q];
    for (int q = 0; q < GSIM_NET_CLASSES; ++q) sf += out[0].first_from[q];
    CHECK(sh == out[0].received && sf == out[0].received - out[0].own);
    CHECK(out[1].peers == 3 && out[1].expected == 15 && out[1].received == 2 && out[1].missed == 15);
    CHECK(out[1].received + out[1].missed > out[1].expected && out[1].lat_max == 4);
    CHECK(out[2].peers == 14 && out[2].messages == 3 && out[2].expected == 42 && out[2].received == 0 && out[2].lat_max == 0);
    CHECK(out[3].peers == 1 && out[3].received == 1 && out[3].hist[1] == 1 && out[3].first_from[0] == 1 && out[3].lat_max == 1);

    // one part: a copy
    {
        std::vector<std::vector<Row>> one(1, parts[0]);
        CHECK(merge(one, {8}, &out) == GSIM_OK);
        CHECK(std::memcmp(out.data(), parts[0].data(), sizeof(Row) * 4) == 0);
    }
    // no rows, no parts
    {
        std::vector<std::vector<Row>> empty(2);
        CHECK(merge(empty, {0, 0}, &out) == GSIM_OK && out.empty());
        std::vector<std::vector<Row>> none;
        CHECK(merge(none, {}, &out) == GSIM_OK);
    }
    // sums past 32 bits stay exact
    {
        std::vector<std::vector<Row>> big(2, std::vector<Row>(1, row(0, 0, 4000000, 4000)));
        big[0][0].lat_sum = big[1][0].lat_sum = 0xC0000000ull;
        big[0][0].hist[31] = big[1][0].hist[31] = 0xF0000000ull;
        CHECK(merge(big, {4000, 4000}, &out) == GSIM_OK);
        CHECK(out[0].expected == 32000000000ull && out[0].lat_sum == 0x180000000ull && out[0].hist[31] == 0x1E0000000ull);
    }
    // disagreements are refused: a row's key, its messages, the selected count
    {
        auto bad = parts;
        bad[1][2].cls = 1;
        CHECK(merge(bad, nm, &out) == GSIM_ESTATE);
        bad = parts;
        bad[2][1].topic = 1;
        CHECK(merge(bad, nm, &out) == GSIM_ESTATE);
        bad = parts;
        bad[1][0].messages = 4;
        CHECK(merge(bad, nm, &out) == GSIM_ESTATE);
        CHECK(merge(parts, {8, 8, 7}, &out) == GSIM_ESTATE);
    }
    if (fails) return 1;
    std::printf("peer report merge ok\n");
    return 0;
}

}  // namespace peer_check

// ---- the score report: merge_score_reports ----
namespace score_check {

using Part = struct gsim_score_part_row;
using Cause = struct gsim_score_cause_row;
using Topic = struct gsim_score_topic_row;

struct Rep {
    std::vector<Part> parts;
    std::vector<Cause> causes;
    std::vector<Topic> topics;
};

// an empty report of C classes and T topics, keys set, min / max at the identities
static Rep empty_report(uint32_t C, uint32_t T)
{
    Rep r;
    for (uint32_t a = 0; a < C; ++a)
        for (uint32_t b = 0; b < C; ++b) {
            for (uint32_t k = 0; k < GSIM_SR_PARTS; ++k) {
                Part p;
                std::memset(&p, 0, sizeof p);
                p.obs_cls = a; p.subj_cls = b; p.part = k;
                p.min = kInf; p.max = -kInf;
                r.parts.push_back(p);
            }
            Cause c;
            std::memset(&c, 0, sizeof c);
            c.obs_cls = a; c.subj_cls = b;
            r.causes.push_back(c);
        }
    for (uint32_t t = 0; t < T; ++t)
        for (uint32_t a = 0; a < C; ++a)
            for (uint32_t b = 0; b < C; ++b) {
                Topic x;
                std::memset(&x, 0, sizeof x);
                x.topic = t; x.obs_cls = a; x.subj_cls = b;
                r.topics.push_back(x);
            }
    return r;
}

static void value(Part& p, int bin, double v)
{
    p.hist[bin] += 1;
    if (v < p.min) p.min = v;
    if (v > p.max) p.max = v;
}

static int merge(const std::vector<Rep>& reps, bool wp, bool wc, bool wt, Rep* out)
{
    std::vector<const Part*> pp;
    std::vector<const Cause*> cp;
    std::vector<const Topic*> tp;
    for (auto& r : reps) { pp.push_back(r.parts.data()); cp.push_back(r.causes.data()); tp.push_back(r.topics.data()); }
    const size_t np = wp ? reps[0].parts.size() : 0, nc = wc ? reps[0].causes.size() : 0, nt = wt ? reps[0].topics.size() : 0;
    out->parts.assign(np, Part{});
    out->causes.assign(nc, Cause{});
    out->topics.assign(nt, Topic{});
    return gsim::merge_score_reports(wp ? pp.data() : nullptr, wc ? cp.data() : nullptr, wt ? tp.data() : nullptr,
                                     reps.size(), np, nc, nt, wp ? out->parts.data() : nullptr,
                                     wc ? out->causes.data() : nullptr, wt ? out->topics.data() : nullptr);
}

static int run()
{
    // three shards, two classes, two topics
    std::vector<Rep> reps;
    for (int l = 0; l < 3; ++l) reps.push_back(empty_report(2, 2));
    const int P3 = GSIM_SR_P3, TOT = GSIM_SR_TOTAL;
    // pair (0, 0): values of P3 and TOTAL on every shard
    value(reps[0].parts[P3], 10, -3.5);
    value(reps[1].parts[P3], 0, -kInf);
    value(reps[2].parts[P3], 16, -0.0);
    value(reps[0].parts[TOT], 20, 0.75);
    value(reps[2].parts[TOT], 32, kInf);
    reps[1].parts[TOT].nan = 2;
    // pair (1, 1): one shard only
    value(reps[1].parts[3 * GSIM_SR_PARTS + TOT], 16, -0.0);
    reps[0].causes[0].connected = 3; reps[0].causes[0].cause[2][0] = 2; reps[0].causes[0].cause[15][6] = 1;
    reps[1].causes[0].connected = 4; reps[1].causes[0].cause[2][0] = 1; reps[1].causes[0].cause[0][5] = 1;
    reps[1].causes[0].nan = 2; reps[1].causes[0].capped = 1;
    reps[2].causes[0].retained = 5; reps[2].causes[0].capped = 2;
    reps[0].topics[4].in_mesh = 7; reps[0].topics[4].negative = 1;
    reps[2].topics[4].in_mesh = 3; reps[2].topics[4].p1_capped = 2; reps[2].topics[4].first_at_cap = 4;
    reps[1].topics[7].active = 6; reps[1].topics[7].p3_deficit = 5; reps[1].topics[7].p3b_nonzero = 4;
    reps[1].topics[7].p4_nonzero = 9;

    Rep out;
    CHECK(merge(reps, true, true, true, &out) == GSIM_OK);
    CHECK(out.parts.size() == 40 && out.causes.size() == 4 && out.topics.size() == 8);
    CHECK(out.parts[P3].obs_cls == 0 && out.parts[P3].subj_cls == 0 && out.parts[P3].part == (uint32_t)P3);
    CHECK(out.parts[P3].hist[10] == 1 && out.parts[P3].hist[0] == 1 && out.parts[P3].hist[16] == 1);
    CHECK(out.parts[P3].min == -kInf && out.parts[P3].max == 0.0 && std::signbit(out.parts[P3].max));
    CHECK(out.parts[TOT].hist[20] == 1 && out.parts[TOT].hist[32] == 1 && out.parts[TOT].nan == 2);
    CHECK(out.parts[TOT].min == 0.75 && out.parts[TOT].max == kInf);
    // a (pair, part) nobody has a value of keeps the identities
    CHECK(out.parts[0].min == kInf && out.parts[0].max == -kInf && out.parts[0].nan == 0);
    CHECK(out.parts[GSIM_SR_PARTS + TOT].min == kInf && out.parts[GSIM_SR_PARTS + TOT].max == -kInf);
    // a pair only one shard has: that shard's min and max
    const Part& p11 = out.parts[3 * GSIM_SR_PARTS + TOT];
    CHECK(p11.obs_cls == 1 && p11.subj_cls == 1 && p11.hist[16] == 1 && p11.min == 0.0 && std::signbit(p11.min) && p11.max == 0.0);
    CHECK(out.causes[0].connected == 7 && out.causes[0].retained == 5 && out.causes[0].nan == 2 && out.causes[0].capped == 3);
    CHECK(out.causes[0].cause[2][0] == 3 && out.causes[0].cause[15][6] == 1 && out.causes[0].cause[0][5] == 1);
    uint64_t sum = 0;
    for (int b = 0; b < GSIM_NET_SCORE_BINS; ++b)
        for (int c = 0; c < GSIM_SR_CAUSES; ++c) sum += out.causes[0].cause[b][c];
    CHECK(sum + out.causes[0].nan == out.causes[0].connected);
    CHECK(out.causes[3].obs_cls == 1 && out.causes[3].subj_cls == 1 && out.causes[3].connected == 0);
    CHECK(out.topics[4].topic == 1 && out.topics[4].obs_cls == 0 && out.topics[4].subj_cls == 0);
    CHECK(out.topics[4].in_mesh == 10 && out.topics[4].p1_capped == 2 && out.topics[4].first_at_cap == 4 &&
          out.topics[4].negative == 1 && out.topics[4].active == 0);
    CHECK(out.topics[7].active == 6 && out.topics[7].p3_deficit == 5 && out.topics[7].p3b_nonzero == 4 &&
          out.topics[7].p4_nonzero == 9 && out.topics[7].in_mesh == 0);

    // one shard: a copy
    {
        std::vector<Rep> one(1, reps[0]);
        CHECK(merge(one, true, true, true, &out) == GSIM_OK);
        CHECK(std::memcmp(out.parts.data(), reps[0].parts.data(), sizeof(Part) * out.parts.size()) == 0);
        CHECK(std::memcmp(out.causes.data(), reps[0].causes.data(), sizeof(Cause) * out.causes.size()) == 0);
        CHECK(std::memcmp(out.topics.data(), reps[0].topics.data(), sizeof(Topic) * out.topics.size()) == 0);
    }
    // each third alone; no rows at all
    {
        CHECK(merge(reps, true, false, false, &out) == GSIM_OK && out.parts[P3].hist[0] == 1 && out.causes.empty());
        CHECK(merge(reps, false, true, false, &out) == GSIM_OK && out.causes[0].connected == 7 && out.topics.empty());
        CHECK(merge(reps, false, false, true, &out) == GSIM_OK && out.topics[4].in_mesh == 10 && out.parts.empty());
        CHECK(merge(reps, false, false, false, &out) == GSIM_OK);
    }
    // disagreements about a row's key are refused
    {
        auto bad = reps;
        bad[1].parts[5].part = 6;
        CHECK(merge(bad, true, true, true, &out) == GSIM_ESTATE);
        bad = reps;
        bad[2].parts[12].subj_cls = 0;
        CHECK(merge(bad, true, true, true, &out) == GSIM_ESTATE);
        bad = reps;
        bad[2].causes[1].obs_cls = 1;
        CHECK(merge(bad, true, true, true, &out) == GSIM_ESTATE);
        bad = reps;
        bad[1].topics[3].topic = 1;
        CHECK(merge(bad, true, true, true, &out) == GSIM_ESTATE);
        bad = reps;
        bad[1].topics[6].subj_cls = 1;
        CHECK(merge(bad, false, false, true, &out) == GSIM_ESTATE);
        // ... but only in the thirds that are merged
        CHECK(merge(bad, true, true, false, &out) == GSIM_OK);
    }
    if (fails) return 1;
    std::printf("score report merge ok\n");
    return 0;
}

}  // namespace score_check

// ---- the mesh path report: merge_mesh_paths ----
namespace mesh_paths_check {

using Row = struct gsim_mesh_path_row;

// a part's row: the shard owns members[c] subscribers of class c
static Row row(uint32_t source, uint32_t topic, const uint32_t (&members)[GSIM_NET_CLASSES])
{
    Row r;
    std::memset(&r, 0, sizeof r);
    r.source = source; r.topic = topic;
    for (int c = 0; c < GSIM_NET_CLASSES; ++c) { r.members_cls[c] = members[c]; r.subscribers += members[c]; }
    return r;
}

// an owned peer of class c reached at distance d
static void reach(Row& r, uint32_t d, int c)
{
    r.reached += 1;
    r.reached_cls[c] += 1;
    r.hist[d < GSIM_REPORT_BINS - 1 ? d : GSIM_REPORT_BINS - 1] += 1;
    if (d > r.max_hops) r.max_hops = d;
}

static int merge(const std::vector<std::vector<Row>>& parts, std::vector<Row>* out)
{
    std::vector<const Row*> pp;
    for (auto& p : parts) pp.push_back(p.data());
    const size_t n = parts.empty() ? 0 : parts[0].size();
    out->assign(n, Row{});
    return gsim::merge_mesh_paths(pp.data(), parts.size(), n, out->data());
}

static int run()
{
    // three shards, three sources of topic 2; the shards own 5 + 2, 4 + 0 and 0 + 3 subscribers of classes 0 and 1
    const uint32_t mem[3][GSIM_NET_CLASSES] = {{5, 2, 0, 0}, {4, 0, 0, 0}, {0, 3, 0, 0}};
    const uint32_t src[3] = {17, 4, 17};                   // a duplicated source
    std::vector<std::vector<Row>> parts(3);
    for (int l = 0; l < 3; ++l)
        for (int k = 0; k < 3; ++k) parts[l].push_back(row(src[k], 2, mem[l]));
    reach(parts[0][0], 0, 0); reach(parts[0][0], 1, 1); reach(parts[0][0], 33, 0);
    reach(parts[1][0], 2, 0); reach(parts[1][0], 40, 0);   // the overflow bin; the largest distance
    reach(parts[2][0], 31, 1);
    parts[1][0].truncated = 1;
    reach(parts[2][1], 0, 1);                              // only one shard reaches anything from source 4
    for (int l = 0; l < 3; ++l) parts[l][2] = parts[l][0]; // the duplicate's rows are equal
    std::vector<Row> out;
    CHECK(merge(parts, &out) == GSIM_OK);
    CHECK(out.size() == 3);
    CHECK(out[0].source == 17 && out[0].topic == 2 && out[1].source == 4);
    CHECK(out[0].reached == 6 && out[0].subscribers == 14 && out[0].max_hops == 40 && out[0].truncated == 1);
    CHECK(out[0].reached_cls[0] == 4 && out[0].reached_cls[1] == 2 && out[0].reached_cls[2] == 0);
    CHECK(out[0].members_cls[0] == 9 && out[0].members_cls[1] == 5 && out[0].members_cls[3] == 0);
    CHECK(out[0].hist[0] == 1 && out[0].hist[1] == 1 && out[0].hist[2] == 1 && out[0].hist[31] == 3);
    uint32_t s = 0;
    for (int q = 0; q < GSIM_REPORT_BINS; ++q) s += out[0].hist[q];
    CHECK(s == out[0].reached);
    CHECK(out[1].reached == 1 && out[1].max_hops == 0 && out[1].truncated == 0 && out[1].subscribers == 14);
    CHECK(out[1].reached_cls[1] == 1 && out[1].hist[0] == 1);
    CHECK(std::memcmp(&out[0], &out[2], sizeof(Row)) == 0);

    // one part: a copy; no rows at all
    {
        std::vector<std::vector<Row>> one(1, parts[0]);
        CHECK(merge(one, &out) == GSIM_OK);
        CHECK(std::memcmp(out.data(), parts[0].data(), sizeof(Row) * 3) == 0);
        std::vector<std::vector<Row>> none(2);
        CHECK(merge(none, &out) == GSIM_OK && out.empty());
    }
    // truncated is an OR, not a sum
    {
        auto both = parts;
        both[0][0].truncated = 1;
        both[2][0].truncated = 1;
        both[0][2].truncated = 1; both[1][2].truncated = 1; both[2][2].truncated = 1;
        CHECK(merge(both, &out) == GSIM_OK && out[0].truncated == 1 && out[2].truncated == 1);
    }
    // disagreements are refused: a row's source or topic between the parts ...
    {
        auto bad = parts;
        bad[1][1].source = 5;
        CHECK(merge(bad, &out) == GSIM_ESTATE);
        bad = parts;
        for (int k = 0; k < 3; ++k) bad[2][k].topic = 1;
        CHECK(merge(bad, &out) == GSIM_ESTATE);
        // ... the topic or the subscriber counts between the rows of one part
        bad = parts;
        bad[1][2].topic = 3;
        CHECK(merge(bad, &out) == GSIM_ESTATE);
        bad = parts;
        bad[0][1].subscribers += 1;
        CHECK(merge(bad, &out) == GSIM_ESTATE);
        bad = parts;
        bad[2][2].members_cls[1] -= 1; bad[2][2].members_cls[2] += 1;      // the same sum, other classes
        CHECK(merge(bad, &out) == GSIM_ESTATE);
    }
    if (fails) return 1;
    std::printf("mesh paths merge ok\n");
    return 0;
}

}  // namespace mesh_paths_check

// ---- the relay report: merge_relay_reports ----
namespace relay_check {

using Row = struct gsim_relay_class_row;

static Row row(uint32_t topic, uint32_t cls, uint32_t peers, uint32_t messages)
{
    Row r;
    std::memset(&r, 0, sizeof r);
    r.topic = topic; r.cls = cls; r.peers = peers; r.messages = messages;
    return r;
}

// one holder (q, m) of the row's class with `children` children, all of class `to`
static void holder(Row& r, uint32_t children, int to)
{
    r.held += 1;
    r.fanout[children < GSIM_REPORT_BINS - 1 ? children : GSIM_REPORT_BINS - 1] += 1;
    if (!children) return;
    r.relayed += 1;
    r.children += children;
    r.children_to[to] += children;
    if (children > r.max_children) r.max_children = children;
}

static int merge(const std::vector<std::vector<Row>>& parts, const std::vector<int64_t>& nm, std::vector<Row>* out)
{
    std::vector<const Row*> pp;
    for (auto& p : parts) pp.push_back(p.data());
    const size_t rows = parts.empty() ? 0 : parts[0].size();
    out->assign(rows, Row{});
    return gsim::merge_relay_reports(pp.data(), nm.data(), parts.size(), rows, out->data());
}

static int run()
{
    CHECK(sizeof(Row) == 336 && sizeof(struct gsim_relay_row) == 64 && sizeof(struct gsim_relay_msg_row) == 216);
    // three shards, two topics x two classes; topic 0 has 5 selected messages, topic 1 has 3
    std::vector<std::vector<Row>> parts(3);
    const uint32_t peers[3][4] = {{10, 2, 7, 0}, {20, 0, 7, 1}, {30, 1, 0, 0}};
    for (int l = 0; l < 3; ++l)
        for (uint32_t t = 0; t < 2; ++t)
            for (uint32_t c = 0; c < 2; ++c) parts[l].push_back(row(t, c, peers[l][t * 2 + c], t == 0 ? 5 : 3));
    std::vector<int64_t> nm(3, 8);
    holder(parts[0][0], 0, 0);             // a leaf
    holder(parts[0][0], 2, 0);
    holder(parts[0][0], 40, 1);            // the overflow bin; the widest holder
    holder(parts[1][0], 3, 1);
    holder(parts[2][0], 33, 0);
    holder(parts[1][3], 1, 0);             // the only part with a holder in row (1, 1)
    holder(parts[2][1], 0, 0);
    holder(parts[2][1], 0, 0);
    std::vector<Row> out;
    CHECK(merge(parts, nm, &out) == GSIM_OK);
    CHECK(out.size() == 4);
    CHECK(out[0].topic == 0 && out[0].cls == 0 && out[3].topic == 1 && out[3].cls == 1);
    CHECK(out[0].peers == 60 && out[0].messages == 5);
    CHECK(out[0].held == 5 && out[0].relayed == 4 && out[0].children == 78 && out[0].max_children == 40);
    CHECK(out[0].fanout[0] == 1 && out[0].fanout[2] == 1 && out[0].fanout[3] == 1 && out[0].fanout[31] == 2);
    CHECK(out[0].children_to[0] == 35 && out[0].children_to[1] == 43 && out[0].children_to[2] == 0);
    uint64_t sf = 0, st = 0;
    for (int q = 0; q < GSIM_REPORT_BINS; ++q) sf += out[0].fanout[q];
    for (int q = 0; q < GSIM_NET_CLASSES; ++q) st += out[0].children_to[q];
    CHECK(sf == out[0].held && st == out[0].children && out[0].held - out[0].fanout[0] == out[0].relayed);
    CHECK(out[1].peers == 3 && out[1].held == 2 && out[1].relayed == 0 && out[1].fanout[0] == 2 && out[1].max_children == 0);
    CHECK(out[2].peers == 14 && out[2].messages == 3 && out[2].held == 0 && out[2].children == 0);
    CHECK(out[3].peers == 1 && out[3].held == 1 && out[3].fanout[1] == 1 && out[3].children_to[0] == 1 && out[3].max_children == 1);

    // one part: a copy
    {
        std::vector<std::vector<Row>> one(1, parts[0]);
        CHECK(merge(one, {8}, &out) == GSIM_OK);
        CHECK(std::memcmp(out.data(), parts[0].data(), sizeof(Row) * 4) == 0);
    }
    // no rows, no parts
    {
        std::vector<std::vector<Row>> empty(2);
        CHECK(merge(empty, {0, 0}, &out) == GSIM_OK && out.empty());
        std::vector<std::vector<Row>> none;
        CHECK(merge(none, {}, &out) == GSIM_OK);
    }
    // sums past 32 bits stay exact
    {
        std::vector<std::vector<Row>> big(2, std::vector<Row>(1, row(0, 0, 4000000, 4000)));
        big[0][0].children = big[1][0].children = 0xC0000000ull;
        big[0][0].children_to[3] = big[1][0].children_to[3] = 0xC0000000ull;
        big[0][0].fanout[31] = big[1][0].fanout[31] = 0xF0000000ull;
        big[0][0].held = big[1][0].held = 0xF0000000ull;
        CHECK(merge(big, {4000, 4000}, &out) == GSIM_OK);
        CHECK(out[0].peers == 8000000 && out[0].children == 0x180000000ull && out[0].children_to[3] == 0x180000000ull);
        CHECK(out[0].fanout[31] == 0x1E0000000ull && out[0].held == 0x1E0000000ull);
    }
    // disagreements are refused: a row's key, its messages, the selected count
    {
        auto bad = parts;
        bad[1][2].cls = 1;
        CHECK(merge(bad, nm, &out) == GSIM_ESTATE);
        bad = parts;
        bad[2][1].topic = 1;
        CHECK(merge(bad, nm, &out) == GSIM_ESTATE);
        bad = parts;
        bad[1][0].messages = 4;
        CHECK(merge(bad, nm, &out) == GSIM_ESTATE);
        CHECK(merge(parts, {8, 8, 7}, &out) == GSIM_ESTATE);
    }
    if (fails) return 1;
    std::printf("relay report merge ok\n");
    return 0;
}

}  // namespace relay_check

int main(int argc, char** argv)
{
    const struct { const char* name; int (*run)(); } sections[] = {
        {"msg", msg_check::run}, {"net", net_check::run}, {"peer", peer_check::run},
        {"score", score_check::run}, {"mesh_paths", mesh_paths_check::run}, {"relay", relay_check::run},
    };
    int ran = 0, rc = 0;
    for (const auto& s : sections)
        if (argc < 2 || !std::strcmp(argv[1], s.name)) {
            rc |= s.run();
            ++ran;
        }
    if (!ran) {
        std::printf("no such section: %s\n", argv[1]);
        return 2;
    }
    return rc;
}
