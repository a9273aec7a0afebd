// paged.h — what the host side (index.hip) and the paged scan's translation units
// (scan_paged.h) share: the paged scan's arguments and its launchers' declarations.
#pragma once

#include "index_common.h"

namespace rc {

// The contiguous scan's arguments read in position space (n_rows = the positions [0, n_pos) of
// this shard; rows_per_block, mask and the keys are over positions), plus the device-resident
// page table: ceil(n_pos / RC_PAGE_ROWS) int32 page numbers, each below capacity / RC_PAGE_ROWS.
// Raw queries only (qraw; qn is not used).  With flags (f16 / bf16 rows): the paged batched
// search's exact fallback, grid.y striding over the flagged queries as in ScanArgs.
struct PagedScanArgs {
    ScanArgs scan;
    const int32_t *pages;
};

template <typename T>
void launch_scan_paged(const PagedScanArgs &p);  // scan_paged.h; instantiated in scan_paged_{f32,f16,bf16,f8}.hip
template <typename T>
void launch_scan_paged_metric(const PagedScanArgs &p);  // ... in scan_paged_metric_{f32,f16,bf16,f8}.hip

}  // namespace rc
