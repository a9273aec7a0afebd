// scan_paged_metric_bf16.hip — instantiates the dotproduct / euclidean page-table scan + top-k for bf16 pool rows.
#include "scan_paged.h"

namespace rc {
template void launch_scan_paged_metric<bf16_t>(const PagedScanArgs &p);
}  // namespace rc
