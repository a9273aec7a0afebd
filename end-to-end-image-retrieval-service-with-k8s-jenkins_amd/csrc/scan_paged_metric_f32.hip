// scan_paged_metric_f32.hip — instantiates the dotproduct / euclidean page-table scan + top-k for f32 pool rows.
#include "scan_paged.h"

namespace rc {
template void launch_scan_paged_metric<float>(const PagedScanArgs &p);
}  // namespace rc
