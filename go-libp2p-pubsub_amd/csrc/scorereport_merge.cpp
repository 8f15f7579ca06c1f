// The host-side merge of the shards' score reports (scorereport_merge.h).
#include "scorereport_merge.h"

namespace gsim {

int merge_score_reports(const gsim_score_part_row* const* part_parts, const gsim_score_cause_row* const* cause_parts,
                        const gsim_score_topic_row* const* topic_parts, size_t n_shards, size_t n_parts, size_t n_causes,
                        size_t n_topics, gsim_score_part_row* part_out, gsim_score_cause_row* cause_out,
                        gsim_score_topic_row* topic_out)
{
    if (part_parts && part_out)
        for (size_t l = 0; l < n_shards; ++l)
            for (size_t k = 0; k < n_parts; ++k) {
                const gsim_score_part_row& x = part_parts[l][k];
                if (l == 0) { part_out[k] = x; continue; }
                gsim_score_part_row& m = part_out[k];
                if (m.obs_cls != x.obs_cls || m.subj_cls != x.subj_cls || m.part != x.part) return GSIM_ESTATE;
                m.nan += x.nan;
                if (x.min < m.min) m.min = x.min;
                if (x.max > m.max) m.max = x.max;
                for (int q = 0; q < GSIM_SR_BINS; ++q) m.hist[q] += x.hist[q];
            }
    if (cause_parts && cause_out)
        for (size_t l = 0; l < n_shards; ++l)
            for (size_t k = 0; k < n_causes; ++k) {
                const gsim_score_cause_row& x = cause_parts[l][k];
                if (l == 0) { cause_out[k] = x; continue; }
                gsim_score_cause_row& m = cause_out[k];
                if (m.obs_cls != x.obs_cls || m.subj_cls != x.subj_cls) return GSIM_ESTATE;
                m.connected += x.connected;
                m.retained += x.retained;
                m.nan += x.nan;
                m.capped += x.capped;
                for (int b = 0; b < GSIM_NET_SCORE_BINS; ++b)
                    for (int c = 0; c < GSIM_SR_CAUSES; ++c) m.cause[b][c] += x.cause[b][c];
            }
    if (topic_parts && topic_out)
        for (size_t l = 0; l < n_shards; ++l)
            for (size_t k = 0; k < n_topics; ++k) {
                const gsim_score_topic_row& x = topic_parts[l][k];
                if (l == 0) { topic_out[k] = x; continue; }
                gsim_score_topic_row& m = topic_out[k];
                if (m.topic != x.topic || m.obs_cls != x.obs_cls || m.subj_cls != x.subj_cls) return GSIM_ESTATE;
                m.in_mesh += x.in_mesh;
                m.p1_capped += x.p1_capped;
                m.first_at_cap += x.first_at_cap;
                m.active += x.active;
                m.p3_deficit += x.p3_deficit;
                m.p3b_nonzero += x.p3b_nonzero;
                m.p4_nonzero += x.p4_nonzero;
                m.negative += x.negative;
            }
    return GSIM_OK;
}

}  // namespace gsim
