// scorereport_merge.h — the host-side merge of the shards' score reports
// (gsim_group_score_report, shard.hip).  Plain host code over include/gsim.h
// alone, so it also builds into a stand-alone program under the host
// sanitizers (tools/scorereport_merge_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "gsim.h"

namespace gsim {

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

}  // namespace gsim
