// Stand-alone check of the host-side merge of the shards' mesh path rows
// (go-libp2p-pubsub_amd/csrc/meshpaths_merge.cpp), meant for the host sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Igo-libp2p-pubsub_amd/csrc tools/meshpaths_merge_check.cpp \
//       go-libp2p-pubsub_amd/csrc/meshpaths_merge.cpp -o meshpaths_merge_check && ./meshpaths_merge_check
//
// Exit status 0 and "mesh paths merge ok" when every case holds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "meshpaths_merge.h"

using Row = struct gsim_mesh_path_row;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

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

int main()
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
