// scan_paged_bf16.hip — instantiates the page-table scan + top-k for bf16 pool rows.
#include "scan_paged.h"

namespace rc {
template void launch_scan_paged<bf16_t>(const PagedScanArgs &p);
}  // namespace rc
