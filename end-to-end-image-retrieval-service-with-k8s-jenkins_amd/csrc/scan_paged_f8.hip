// scan_paged_f8.hip — instantiates the page-table scan + top-k for f8 pool rows.
#include "scan_paged.h"

namespace rc {
template void launch_scan_paged<f8_t>(const PagedScanArgs &p);
}  // namespace rc
