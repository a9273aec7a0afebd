// scan_metric_bf16.hip — instantiates the dotproduct / euclidean scan + top-k for bf16 index rows.
#include "scan_metric.h"

namespace rc {
template void launch_scan_metric<bf16_t>(const ScanArgs &a);
template void launch_query1_metric_scan<bf16_t>(const Query1Args &a, hipStream_t s);
}  // namespace rc
