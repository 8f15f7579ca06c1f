// The host-side merge of the shards' propagation reports (report_merge.h).
#include "report_merge.h"

namespace gsim {

int merge_reports(const struct ::gsim_msg_report* const* parts, const uint32_t* const* gid, const size_t* gid_n,
                  size_t n_parts, size_t rows, struct ::gsim_msg_report* out)
{
    constexpr uint32_t kNoPeer = 0xFFFFFFFFu;
    for (size_t l = 0; l < n_parts; ++l) {
        for (size_t k = 0; k < rows; ++k) {
            struct ::gsim_msg_report x = parts[l][k];
            if (x.origin != kNoPeer) {
                if ((size_t)x.origin >= gid_n[l]) return GSIM_ESTATE;
                x.origin = gid[l][x.origin];
            }
            if (l == 0) { out[k] = x; continue; }
            struct ::gsim_msg_report& m = out[k];           // every shard orders by (pub_round, slot)
            if (m.slot != x.slot || m.id != x.id || m.pub_round != x.pub_round || m.topic != x.topic ||
                m.verdict != x.verdict || m.vdelay != x.vdelay)
                return GSIM_ESTATE;
            if (m.origin == kNoPeer) m.origin = x.origin;
            else if (x.origin != kNoPeer && x.origin != m.origin) return GSIM_ESTATE;
            for (int q = 0; q < GSIM_REPORT_BINS; ++q) m.hist[q] += x.hist[q];
            m.reached += x.reached;
            m.subscribers += x.subscribers;
            if (x.max_latency > m.max_latency) m.max_latency = x.max_latency;
        }
    }
    return GSIM_OK;
}

}  // namespace gsim
