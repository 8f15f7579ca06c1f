// netreport_merge.h — the host-side merge of the shards' network reports
// (gsim_group_net_report, shard.hip).  Plain host code over include/gsim.h
// alone, so it also builds into a stand-alone program under the host
// sanitizers (tools/netreport_merge_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "gsim.h"

namespace gsim {

// Merge `n_parts` reports (every shard's gsim_net_report over the observers it
// owns) of n_mesh mesh rows and n_scores score rows each into mesh_out /
// score_out: counts and histograms summed, max_degree the maximum, the scores'
// min the minimum and max the maximum (a part without connected non-NaN edges
// holds +inf / -inf, the identities).  Either half may be skipped (parts and out
// NULL, or zero rows).  Returns GSIM_ESTATE (out unspecified) when the parts
// disagree about a row's (topic, cls) or (obs_cls, subj_cls), GSIM_OK otherwise.
int merge_net_reports(const gsim_mesh_row* const* mesh_parts, const gsim_score_row* const* score_parts, size_t n_parts,
                      size_t n_mesh, size_t n_scores, gsim_mesh_row* mesh_out, gsim_score_row* score_out);

}  // namespace gsim
