// The host-side merge of the shards' relay class rows (relayreport_merge.h).
#include "relayreport_merge.h"

namespace gsim {

int merge_relay_reports(const gsim_relay_class_row* const* parts, const int64_t* n_msgs, size_t n_parts, size_t n_rows,
                        gsim_relay_class_row* out)
{
    for (size_t l = 1; l < n_parts; ++l)
        if (n_msgs[l] != n_msgs[0]) return GSIM_ESTATE;
    for (size_t l = 0; l < n_parts; ++l)
        for (size_t k = 0; k < n_rows; ++k) {
            const gsim_relay_class_row& x = parts[l][k];
            if (l == 0) { out[k] = x; continue; }
            gsim_relay_class_row& m = out[k];
            if (m.topic != x.topic || m.cls != x.cls || m.messages != x.messages) return GSIM_ESTATE;
            m.peers += x.peers;
            m.held += x.held;
            m.relayed += x.relayed;
            m.children += x.children;
            if (x.max_children > m.max_children) m.max_children = x.max_children;
            for (int q = 0; q < GSIM_NET_CLASSES; ++q) m.children_to[q] += x.children_to[q];
            for (int q = 0; q < GSIM_REPORT_BINS; ++q) m.fanout[q] += x.fanout[q];
        }
    return GSIM_OK;
}

}  // namespace gsim
