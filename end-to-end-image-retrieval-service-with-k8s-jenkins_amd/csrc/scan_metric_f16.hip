// scan_metric_f16.hip — instantiates the dotproduct / euclidean scan + top-k for f16 index rows.
#include "scan_metric.h"

namespace rc {
template void launch_scan_metric<f16_t>(const ScanArgs &a);
template void launch_query1_metric_scan<f16_t>(const Query1Args &a, hipStream_t s);
}  // namespace rc
