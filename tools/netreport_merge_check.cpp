// Stand-alone check of the host-side merge of the shards' network reports
// (go-libp2p-pubsub_amd/csrc/netreport_merge.cpp), meant for the host sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Igo-libp2p-pubsub_amd/csrc tools/netreport_merge_check.cpp \
//       go-libp2p-pubsub_amd/csrc/netreport_merge.cpp -o netreport_merge_check && ./netreport_merge_check
//
// Exit status 0 and "net report merge ok" when every case holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "netreport_merge.h"

using Mesh = struct gsim_mesh_row;
using Score = struct gsim_score_row;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static const double kInf = std::numeric_limits<double>::infinity();

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

int main()
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
