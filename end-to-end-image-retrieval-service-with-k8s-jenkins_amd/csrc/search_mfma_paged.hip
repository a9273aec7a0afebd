// search_mfma_paged.hip — the page-table forms of the batched search's native (f16 / bf16) filter
// kernels: a named namespace's batched MFMA search (rc_index_search_pages_ex, BatchPlan::pages).
//
// A namespace's vectors are dense in POSITION space [0, n_pos) of a shard and position p lives at
// local row pages[p / RC_PAGE_ROWS] · RC_PAGE_ROWS + p % RC_PAGE_ROWS of the pool's rows
// (scan_paged.h).  The staged search of search_mfma.hip runs over positions unchanged — the same
// stages, sub-launches, block mapping, thresholds, candidate lists (of positions), bitmap (over
// positions) and `row < r_end` tests — and its kernels here are the same bodies
// (filter_qs_body.inc, filter_gemm_body.inc) with PAGED set: the row tile's DMA base and, under
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
#include "filter_mfma.h"
#include "paged.h"

namespace rc {

// METRIC and MASKED as template parameters: new kernels, so the parameters cost no existing symbol
// (fm is not read without METRIC, mask not without MASKED).
// Not instantiated: filter_qs_paged_kernel<T, 8, true, true> (ld 512, METRIC and MASKED).  The
// contiguous form of it sits at 256 VGPRs with nothing to spare, and with the page words it needs 8
// bytes of scratch (tools/kernel_resources.py), also when the epilogue's page is loaded in the epilogue
// itself.  paged_filter_supported says so to the callers: RC_SEARCH_MFMA_MASKED with a mask is
// refused there (RC_ERR_UNSUPPORTED), and RC_SEARCH_AUTO with a mask scans in any case.
bool paged_filter_supported(int64_t ld, bool metric, bool mask_filter) { return !(ld == 512 && metric && mask_filter); }

template <typename T, int NKT, bool METRIC, bool MASKED>
__global__ __launch_bounds__(512, 1) void filter_qs_paged_kernel(FilterArgs a, FilterMetric fm, const uint32_t *mask,
                                                                 const int32_t *pages) {
    constexpr bool PAGED = true;
    constexpr int ABL = 0;
#include "filter_qs_body.inc"
}
template <typename T, bool METRIC, bool MASKED>
__global__ __launch_bounds__(512, 1) void filter_gemm_paged_kernel(FilterArgs a, FilterMetric fm, const uint32_t *mask,
                                                                   const int32_t *pages) {
    constexpr bool PAGED = true;
#include "filter_gemm_body.inc"
}

// One filter dispatch of run_stages over positions [fa.r_begin, fa.r_end) in nchunk chunks
// (run_batched's lambda hands it over when the plan has a page table): the kernel choice by row
// width is the contiguous search's.
template <typename T>
void launch_filter_paged(const BatchPlan &p, const BatchWs &ws, FilterArgs fa, int64_t nchunk, int nqb, hipStream_t s) {
    const int nkt = (int)(p.ld / 64);
    const FilterMetric fm{p.norms, ws.mcoef};
    const dim3 gr((unsigned)(nchunk * nqb)), bl(512);
    auto launch = [&](auto metric, auto masked) {
        constexpr bool ME = decltype(metric)::value, MA = decltype(masked)::value;
        if (nkt == 2 || nkt == 4 || nkt == 8) {
            fa.tiles_per_chunk = ((fa.r_end - fa.r_begin + QS_RT - 1) / QS_RT + nchunk - 1) / nchunk;
            if (nkt == 8) {
                if constexpr (ME && MA) throw Error(RC_ERR_UNSUPPORTED, "no paged metric filter with the mask inside at ld 512");
                else hipLaunchKernelGGL((filter_qs_paged_kernel<T, 8, ME, MA>), gr, bl, 0, s, fa, fm, p.mask, p.pages);
            } else if (nkt == 4) hipLaunchKernelGGL((filter_qs_paged_kernel<T, 4, ME, MA>), gr, bl, 0, s, fa, fm, p.mask, p.pages);
            else hipLaunchKernelGGL((filter_qs_paged_kernel<T, 2, ME, MA>), gr, bl, 0, s, fa, fm, p.mask, p.pages);
        } else {
            hipLaunchKernelGGL((filter_gemm_paged_kernel<T, ME, MA>), gr, bl, 0, s, fa, fm, p.mask, p.pages);
        }
    };
    auto with_mask = [&](auto metric) {
        if (p.mask_filter) launch(metric, std::true_type{});
        else launch(metric, std::false_type{});
    };
    if (p.metric != RC_METRIC_COSINE) with_mask(std::true_type{});
    else with_mask(std::false_type{});
}

template void launch_filter_paged<f16_t>(const BatchPlan &, const BatchWs &, FilterArgs, int64_t, int, hipStream_t);
template void launch_filter_paged<bf16_t>(const BatchPlan &, const BatchWs &, FilterArgs, int64_t, int, hipStream_t);

}  // namespace rc
