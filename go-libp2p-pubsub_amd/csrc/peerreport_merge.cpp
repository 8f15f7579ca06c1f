// The host-side merge of the shards' peer delivery class rows (peerreport_merge.h).
#include "peerreport_merge.h"

namespace gsim {

int merge_peer_reports(const gsim_peer_class_row* const* parts, const int64_t* n_msgs, size_t n_parts, size_t n_rows,
                       gsim_peer_class_row* out)
{
    for (size_t l = 1; l < n_parts; ++l)
        if (n_msgs[l] != n_msgs[0]) return GSIM_ESTATE;
    for (size_t l = 0; l < n_parts; ++l)
        for (size_t k = 0; k < n_rows; ++k) {
            const gsim_peer_class_row& x = parts[l][k];
            if (l == 0) { out[k] = x; continue; }
            gsim_peer_class_row& m = out[k];
            if (m.topic != x.topic || m.cls != x.cls || m.messages != x.messages) return GSIM_ESTATE;
            m.peers += x.peers;
            m.expected += x.expected;
            m.received += x.received;
            m.own += x.own;
            m.missed += x.missed;
            m.lat_sum += x.lat_sum;
            if (x.lat_max > m.lat_max) m.lat_max = x.lat_max;
            for (int q = 0; q < GSIM_NET_CLASSES; ++q) m.first_from[q] += x.first_from[q];
            for (int q = 0; q < GSIM_REPORT_BINS; ++q) m.hist[q] += x.hist[q];
        }
    return GSIM_OK;
}

}  // namespace gsim
