// scan_f16.hip — instantiates the streaming scan + top-k for f16 index rows.
#include "scan.h"

namespace rc {
template void launch_scan<f16_t>(const ScanArgs &a);
template void launch_query1<f16_t>(const Query1Args &a, hipStream_t s);
}  // namespace rc
