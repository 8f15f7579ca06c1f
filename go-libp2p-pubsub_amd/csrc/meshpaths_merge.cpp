// The host-side merge of the shards' mesh path rows (meshpaths_merge.h).
#include "meshpaths_merge.h"

namespace gsim {

int merge_mesh_paths(const gsim_mesh_path_row* const* parts, size_t n_parts, size_t n_rows, gsim_mesh_path_row* out)
{
    if (!parts || !out) return n_rows ? GSIM_ESTATE : GSIM_OK;
    for (size_t l = 0; l < n_parts; ++l)
        for (size_t k = 0; k < n_rows; ++k) {
            const gsim_mesh_path_row& x = parts[l][k];
            const gsim_mesh_path_row& x0 = parts[l][0];
            if (x.topic != x0.topic || x.subscribers != x0.subscribers) return GSIM_ESTATE;
            for (int q = 0; q < GSIM_NET_CLASSES; ++q)
                if (x.members_cls[q] != x0.members_cls[q]) return GSIM_ESTATE;
            if (l == 0) { out[k] = x; continue; }
            gsim_mesh_path_row& m = out[k];
            if (m.source != x.source || m.topic != x.topic) return GSIM_ESTATE;
            m.reached += x.reached;
            m.subscribers += x.subscribers;
            if (x.max_hops > m.max_hops) m.max_hops = x.max_hops;
            m.truncated |= x.truncated;
            for (int q = 0; q < GSIM_NET_CLASSES; ++q) {
                m.reached_cls[q] += x.reached_cls[q];
                m.members_cls[q] += x.members_cls[q];
            }
            for (int q = 0; q < GSIM_REPORT_BINS; ++q) m.hist[q] += x.hist[q];
        }
    return GSIM_OK;
}

}  // namespace gsim
