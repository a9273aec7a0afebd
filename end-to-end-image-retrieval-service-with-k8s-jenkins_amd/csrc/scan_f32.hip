// scan_f32.hip — instantiates the streaming scan + top-k for f32 index rows.
#include "scan.h"

namespace rc {
template void launch_scan<float>(const ScanArgs &a);
template void launch_query1<float>(const Query1Args &a, hipStream_t s);
}  // namespace rc
