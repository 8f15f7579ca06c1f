// report_merge.h — the host-side merge of the shards' propagation reports
// (gsim_group_msg_report, shard.hip).  Plain host code over include/gsim.h
// alone, so it also builds into a stand-alone program under the host
// sanitizers (tools/report_merge_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "gsim.h"

namespace gsim {

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

}  // namespace gsim
