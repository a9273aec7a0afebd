// scan_paged_metric_f16.hip — instantiates the dotproduct / euclidean page-table scan + top-k for f16 pool rows.
#include "scan_paged.h"

namespace rc {
template void launch_scan_paged_metric<f16_t>(const PagedScanArgs &p);
}  // namespace rc
