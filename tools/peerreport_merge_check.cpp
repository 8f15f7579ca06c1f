// Stand-alone check of the host-side merge of the shards' peer delivery class
// rows (go-libp2p-pubsub_amd/csrc/peerreport_merge.cpp), meant for the host
// sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Igo-libp2p-pubsub_amd/csrc tools/peerreport_merge_check.cpp \
//       go-libp2p-pubsub_amd/csrc/peerreport_merge.cpp -o peerreport_merge_check && ./peerreport_merge_check
//
// Exit status 0 and "peer report merge ok" when every case holds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "peerreport_merge.h"

using Row = struct gsim_peer_class_row;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

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

int main()
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
