// relayreport_merge.h — the host-side part of gsim_group_relay_report
// (shard.hip): the merge of the shards' relay class rows.  Plain host code over
// include/gsim.h alone, so it also builds into a stand-alone program under the
// host sanitizers (tools/relayreport_merge_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "gsim.h"

namespace gsim {

// Merge `n_parts` reports (every shard's relay class rows over the peers it
// owns, n_rows rows each, with the messages each part selected in n_msgs[l])
// into out: counts, sums and histograms added, max_children the maximum.  Every
// shard sees every publication, so a row's (topic, cls) and messages and the
// selected count are the same in every part: GSIM_ESTATE (out unspecified) when
// they are not, GSIM_OK otherwise.  No parts or no rows: nothing written.
int merge_relay_reports(const gsim_relay_class_row* const* parts, const int64_t* n_msgs, size_t n_parts, size_t n_rows,
                        gsim_relay_class_row* out);

}  // namespace gsim
