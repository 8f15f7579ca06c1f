// The host-side merges of the shards' report rows (report_merge.h).
#include "report_merge.h"

namespace gsim {

// ---- the propagation report (gsim_group_msg_report)

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

// ---- the network report (gsim_group_net_report)

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

// ---- the peer delivery report (gsim_group_peer_report)

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

// ---- the score report (gsim_group_score_report)

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

// ---- the mesh path report (gsim_group_mesh_paths)

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

// ---- the relay report (gsim_group_relay_report)

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
