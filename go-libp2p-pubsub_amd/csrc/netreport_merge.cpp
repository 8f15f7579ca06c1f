// The host-side merge of the shards' network reports (netreport_merge.h).
#include "netreport_merge.h"

namespace gsim {

int merge_net_reports(const gsim_mesh_row* const* mesh_parts, const gsim_score_row* const* score_parts, size_t n_parts,
                      size_t n_mesh, size_t n_scores, gsim_mesh_row* mesh_out, gsim_score_row* score_out)
{
    if (mesh_parts && mesh_out)
        for (size_t l = 0; l < n_parts; ++l)
            for (size_t k = 0; k < n_mesh; ++k) {
                const gsim_mesh_row& x = mesh_parts[l][k];
                if (l == 0) { mesh_out[k] = x; continue; }
                gsim_mesh_row& m = mesh_out[k];
                if (m.topic != x.topic || m.cls != x.cls) return GSIM_ESTATE;
                m.members += x.members;
                m.fanout_peers += x.fanout_peers;
                if (x.max_degree > m.max_degree) m.max_degree = x.max_degree;
                for (int q = 0; q < GSIM_NET_CLASSES; ++q) m.mesh_links[q] += x.mesh_links[q];
                m.outbound_links += x.outbound_links;
                m.fanout_links += x.fanout_links;
                for (int q = 0; q < GSIM_NET_DEG_BINS; ++q) m.deg_hist[q] += x.deg_hist[q];
                for (int q = 0; q < GSIM_NET_OUT_BINS; ++q) m.out_hist[q] += x.out_hist[q];
            }
    if (score_parts && score_out)
        for (size_t l = 0; l < n_parts; ++l)
            for (size_t k = 0; k < n_scores; ++k) {
                const gsim_score_row& x = score_parts[l][k];
                if (l == 0) { score_out[k] = x; continue; }
                gsim_score_row& m = score_out[k];
                if (m.obs_cls != x.obs_cls || m.subj_cls != x.subj_cls) return GSIM_ESTATE;
                m.connected += x.connected;
                m.retained += x.retained;
                m.nan += x.nan;
                if (x.min < m.min) m.min = x.min;
                if (x.max > m.max) m.max = x.max;
                for (int q = 0; q < GSIM_NET_SCORE_BINS; ++q) m.hist[q] += x.hist[q];
            }
    return GSIM_OK;
}

}  // namespace gsim
