// meshpaths_merge.h — the host-side merge of the shards' mesh path rows
// (gsim_group_mesh_paths, shard.hip).  Plain host code over include/gsim.h
// alone, so it also builds into a stand-alone program under the host
// sanitizers (tools/meshpaths_merge_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "gsim.h"

namespace gsim {

// Merge `n_parts` parts (every shard's rows over the peers it owns) of n_rows
// rows each, one per source in the caller's order, into out: reached,
// reached_cls, hist, subscribers and members_cls summed, max_hops the maximum,
// truncated the OR.  Returns GSIM_ESTATE (out unspecified) when the parts
// disagree about a row's source or topic, or when the rows of one part
// disagree about the topic or the subscriber counts (subscribers,
// members_cls: a part counts its owned subscribers of the call's one topic,
// the same for every source); GSIM_OK otherwise.
int merge_mesh_paths(const gsim_mesh_path_row* const* parts, size_t n_parts, size_t n_rows, gsim_mesh_path_row* out);

}  // namespace gsim
