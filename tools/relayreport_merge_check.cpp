// Stand-alone check of the host-side merge of the shards' relay class rows
// (go-libp2p-pubsub_amd/csrc/relayreport_merge.cpp), meant for the host
// sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Igo-libp2p-pubsub_amd/csrc tools/relayreport_merge_check.cpp \
//       go-libp2p-pubsub_amd/csrc/relayreport_merge.cpp -o relayreport_merge_check && ./relayreport_merge_check
//
// Exit status 0 and "relay report merge ok" when every case holds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "relayreport_merge.h"

using Row = struct gsim_relay_class_row;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

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

int main()
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
