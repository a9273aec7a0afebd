// scan_metric_f32.hip — instantiates the dotproduct / euclidean scan + top-k for f32 index rows.
#include "scan_metric.h"

namespace rc {
template void launch_scan_metric<float>(const ScanArgs &a);
template void launch_query1_metric_scan<float>(const Query1Args &a, hipStream_t s);
}  // namespace rc
