// Stand-alone check of the host-side merge of the shards' score reports
// (go-libp2p-pubsub_amd/csrc/scorereport_merge.cpp), meant for the host sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Igo-libp2p-pubsub_amd/csrc tools/scorereport_merge_check.cpp \
//       go-libp2p-pubsub_amd/csrc/scorereport_merge.cpp -o scorereport_merge_check && ./scorereport_merge_check
//
// Exit status 0 and "score report merge ok" when every case holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "scorereport_merge.h"

using Part = struct gsim_score_part_row;
using Cause = struct gsim_score_cause_row;
using Topic = struct gsim_score_topic_row;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static const double kInf = std::numeric_limits<double>::infinity();

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

int main()
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
