// scan_paged_metric_f8.hip — instantiates the dotproduct / euclidean page-table scan + top-k for f8 pool rows.
#include "scan_paged.h"

namespace rc {
template void launch_scan_paged_metric<f8_t>(const PagedScanArgs &p);
}  // namespace rc
