// search_mfma_paged.hip — the page-table forms of the batched search's native (f16 / bf16) filter
// kernels: a named namespace's batched MFMA search (rc_index_search_pages_ex, BatchPlan::pages).
//
// A namespace's vectors are dense in POSITION space [0, n_pos) of a shard and position p lives at
// local row pages[p / RC_PAGE_ROWS] · RC_PAGE_ROWS + p % RC_PAGE_ROWS of the pool's rows
// (scan_paged.h).  The staged search of search_mfma.hip runs over positions unchanged — the same
// stages, sub-launches, block mapping, thresholds, candidate lists (of positions), bitmap (over
// positions) and `row < r_end` tests — and its kernels here are the same kernel templates
// (filter_native.h) with PAGED set: the row tile's DMA base and, under
// METRIC, the tile's norms are the only two addresses that go through the page table, one
// wave-uniform page number per tile (filter_mfma.h, "PAGED forms").  The exact rescoring is
// rescore_paged_kernel (rescore.h) and the overflow fallback scan_topk_paged_fallback_kernel
// (scan_paged.h).
//
// Exactness: the arguments of search_mfma.hip's header and of the METRIC and MASKED epilogues
// (filter_mfma.h) speak of the values s', c, n, thr and of the set of rows seen so far, never of
// where a row is stored.  Position p's row bytes and norm are those of the dense index holding the
// namespace in position order, so every such value is the dense search's and the arguments carry
// over word for word; the results are the paged scan's bits, ties included.
//
// The last tile reads past r_end inside its own page (a page lies wholly inside the pool: the host
// checks every page number), so the rows need no clamp; the norm loads keep theirs to left - 1.
// Rows past r_end in that page may be stale rows of other namespaces: they are scored and never
// appended.
#include "filter_native.h"

namespace rc {

// Every form but ld 512 with METRIC and MASKED (launch_filter_native's comment).  For the callers:
// RC_SEARCH_MFMA_MASKED with a mask is refused there (RC_ERR_UNSUPPORTED), and RC_SEARCH_AUTO with
// a mask scans in any case.
bool paged_filter_supported(int64_t ld, bool metric, bool mask_filter) { return !(ld == 512 && metric && mask_filter); }

template void launch_filter_native<f16_t, true>(const BatchPlan &, const BatchWs &, int64_t, int64_t, int64_t, int, hipStream_t);
template void launch_filter_native<bf16_t, true>(const BatchPlan &, const BatchWs &, int64_t, int64_t, int64_t, int, hipStream_t);

}  // namespace rc
