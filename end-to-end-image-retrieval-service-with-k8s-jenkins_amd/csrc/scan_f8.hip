// scan_f8.hip — instantiates the streaming scan + top-k for float8 (OCP e4m3fn) index rows.
#include "scan.h"

namespace rc {
template void launch_scan<f8_t>(const ScanArgs &a);
template void launch_query1<f8_t>(const Query1Args &a, hipStream_t s);
}  // namespace rc
