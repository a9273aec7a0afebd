// scan_paged_f16.hip — instantiates the page-table scan + top-k for f16 pool rows.
#include "scan_paged.h"

namespace rc {
template void launch_scan_paged<f16_t>(const PagedScanArgs &p);
}  // namespace rc
