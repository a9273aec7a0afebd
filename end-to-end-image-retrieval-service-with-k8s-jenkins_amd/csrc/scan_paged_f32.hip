// scan_paged_f32.hip — instantiates the page-table scan + top-k for f32 pool rows.
#include "scan_paged.h"

namespace rc {
template void launch_scan_paged<float>(const PagedScanArgs &p);
}  // namespace rc
