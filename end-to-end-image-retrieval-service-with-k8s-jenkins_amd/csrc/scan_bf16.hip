// scan_bf16.hip — instantiates the streaming scan + top-k for bf16 index rows.
#include "scan.h"

namespace rc {
template void launch_scan<bf16_t>(const ScanArgs &a);
template void launch_query1<bf16_t>(const Query1Args &a, hipStream_t s);
}  // namespace rc
