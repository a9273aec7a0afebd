// scan_metric_f8.hip — instantiates the dotproduct / euclidean scan + top-k for float8 index rows.
#include "scan_metric.h"

namespace rc {
template void launch_scan_metric<f8_t>(const ScanArgs &a);
template void launch_query1_metric_scan<f8_t>(const Query1Args &a, hipStream_t s);
}  // namespace rc
