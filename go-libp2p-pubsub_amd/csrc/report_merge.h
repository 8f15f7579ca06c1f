// report_merge.h — the host-side merges of the shards' report rows
// (gsim_group_*_report and gsim_group_mesh_paths, shard.hip).  Plain host code
// over include/gsim.h alone, so it also builds into a stand-alone program under
// the host sanitizers (tools/report_merge_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "gsim.h"

namespace gsim {

// ---- the propagation report (gsim_group_msg_report)

// Merge `n_parts` reports of `rows` rows each (every shard's gsim_msg_report
// over the peers it owns, each ordered by (pub_round, slot)) into out[rows]:
// hist, reached and subscribers summed, max_latency the maximum.  A part's
// origin is a local peer id of that shard (gid[l][origin], gid_n[l] entries, is
// its global id) or 0xFFFFFFFF where the publisher is no local peer there; the
// merged origin is the global id from a shard that knows it.  Returns
// GSIM_ESTATE (out unspecified) when the parts disagree about a slot's message
// or an origin lies outside its shard's id table, GSIM_OK otherwise.
int merge_reports(const struct ::gsim_msg_report* const* parts, const uint32_t* const* gid, const size_t* gid_n,
                  size_t n_parts, size_t rows, struct ::gsim_msg_report* out);

// ---- the network report (gsim_group_net_report)

// Merge `n_parts` reports (every shard's gsim_net_report over the observers it
// owns) of n_mesh mesh rows and n_scores score rows each into mesh_out /
// score_out: counts and histograms summed, max_degree the maximum, the scores'
// min the minimum and max the maximum (a part without connected non-NaN edges
// holds +inf / -inf, the identities).  Either half may be skipped (parts and out
// NULL, or zero rows).  Returns GSIM_ESTATE (out unspecified) when the parts
// disagree about a row's (topic, cls) or (obs_cls, subj_cls), GSIM_OK otherwise.
int merge_net_reports(const gsim_mesh_row* const* mesh_parts, const gsim_score_row* const* score_parts, size_t n_parts,
                      size_t n_mesh, size_t n_scores, gsim_mesh_row* mesh_out, gsim_score_row* score_out);

// ---- the peer delivery report (gsim_group_peer_report)

// Merge `n_parts` reports (every shard's gsim_peer_report class rows over the
// peers it owns, n_rows rows each, with the messages each part selected in
// n_msgs[l]) into out: counts, sums and histograms added, lat_max the maximum.
// Every shard sees every publication, so a row's (topic, cls) and messages and
// the selected count are the same in every part: GSIM_ESTATE (out unspecified)
// when they are not, GSIM_OK otherwise.  No parts or no rows: nothing written.
int merge_peer_reports(const gsim_peer_class_row* const* parts, const int64_t* n_msgs, size_t n_parts, size_t n_rows,
                       gsim_peer_class_row* out);

// ---- the score report (gsim_group_score_report)

// Merge `n_shards` reports (every shard's gsim_score_report over the records of
// the observers it owns) of n_parts part rows, n_causes cause rows and n_topics
// topic rows each into the three outputs: counts and histograms summed, a part's
// min the minimum and max the maximum (a shard without connected non-NaN values
// holds +inf / -inf, the identities).  Any third may be skipped (its parts and
// out NULL, or zero rows).  Returns GSIM_ESTATE (out unspecified) when the
// shards disagree about a row's key -- (obs_cls, subj_cls, part), (obs_cls,
// subj_cls) or (topic, obs_cls, subj_cls) -- and GSIM_OK otherwise.
int merge_score_reports(const gsim_score_part_row* const* part_parts, const gsim_score_cause_row* const* cause_parts,
                        const gsim_score_topic_row* const* topic_parts, size_t n_shards, size_t n_parts, size_t n_causes,
                        size_t n_topics, gsim_score_part_row* part_out, gsim_score_cause_row* cause_out,
                        gsim_score_topic_row* topic_out);

// ---- the mesh path report (gsim_group_mesh_paths)

// Merge `n_parts` parts (every shard's rows over the peers it owns) of n_rows
// rows each, one per source in the caller's order, into out: reached,
// reached_cls, hist, subscribers and members_cls summed, max_hops the maximum,
// truncated the OR.  Returns GSIM_ESTATE (out unspecified) when the parts
// disagree about a row's source or topic, or when the rows of one part
// disagree about the topic or the subscriber counts (subscribers,
// members_cls: a part counts its owned subscribers of the call's one topic,
// the same for every source); GSIM_OK otherwise.
int merge_mesh_paths(const gsim_mesh_path_row* const* parts, size_t n_parts, size_t n_rows, gsim_mesh_path_row* out);

// ---- the relay report (gsim_group_relay_report)

// Merge `n_parts` reports (every shard's relay class rows over the peers it
// owns, n_rows rows each, with the messages each part selected in n_msgs[l])
// into out: counts, sums and histograms added, max_children the maximum.  Every
// shard sees every publication, so a row's (topic, cls) and messages and the
// selected count are the same in every part: GSIM_ESTATE (out unspecified) when
// they are not, GSIM_OK otherwise.  No parts or no rows: nothing written.
int merge_relay_reports(const gsim_relay_class_row* const* parts, const int64_t* n_msgs, size_t n_parts, size_t n_rows,
                        gsim_relay_class_row* out);

}  // namespace gsim
