// rescore.h — the batched search's exact rescoring (search_mfma.hip's stages): the device code of
// rescore_kernel and of its metric form, and the metric form's launch.  Included by
// search_mfma.hip, which instantiates the cosine kernels, by rescore_metric_{f16,bf16}.hip,
// which instantiate launch_rescore_metric<T> for one storage dtype each, and by
// rescore_paged_{f16,bf16}.hip, which do the same for the page-table form (launch_rescore_paged<T>): the metric kernels (96
// instantiations) compile in two translation units of their own, in parallel with the rest.
#pragma once

#include "index_common.h"

namespace rc {

// ------------------------------------------------------- exact rescoring --
// One block per query.  Candidates are scored exactly as scan_topk_kernel
// scores a row (RC_ROW_FMA16 + sum16: 16 lanes per row, 16-B chunks, f32 FMA in chunk
// order, DPP reduction), merged with the running top-k keys, and the threshold for the
// next stage is set.  Overflow (more candidates than cap) is flagged for the
// host's exact fallback; the counter is reset for the next stage.
//
// MASKED (rc_index_search_masked; `mask` as in ScanArgs): a candidate whose bit is clear is
// scored but not pushed; the filter kernels are untouched.  Why that is exact: the running
// list then holds eligible rows only, so thr[q] is -inf or (kth best exact score among the
// ELIGIBLE rows seen so far) - eps[q], a lower bound of the final masked kth best minus eps;
// by the header's argument every eligible row of the masked top-k has s' >= thr[q] at its
// stage, passes the filter, and is rescored here.  Ineligible rows only take candidate slots:
// thr rises more slowly than in an unmasked search (it stays -inf until k eligible rows were
// seen), so a selective mask overflows sooner.  An overflowed query is flagged exactly as
// before — n counts every appended candidate, eligible or not, so a list that lost entries
// is never trusted — and the fallback is the MASKED scan (index.hip), whose lists the
// unchanged merge writes over this kernel's output.  Candidate rows are < r_end <= n_rows
// (every filter epilogue tests that), so mask[row >> 5] stays inside the bitmap.
//
// METRIC (rescore_metric_kernel, RC_FILTER_METRIC under dotproduct / euclidean): the key's score
// is metric_score(mc, s, norms[row]) with s the exact cosine above and mc the query's prepared
// constants (mcoef: eps, alpha, beta, gamma) — the scan's rule on the scan's operands (qn is the
// RC_UNIT_ELEM product the metric scan forms), so the scan's bits — and thr[q] is the k-th best
// metric score itself: the filter's u is an upper bound of the exact score with no slack left to
// subtract (the metric epilogue's comment in search_mfma.hip).  The masked argument carries over
// unchanged: the list holds eligible rows only, so thr[q] is a lower bound of the final masked
// k-th best.
// The body is rescore_body.inc, included in both kernels: one copy of the text, and the cosine
// kernels keep the instructions they had.
template <typename T, int NCH, int CAP, bool MASKED>
__global__ __launch_bounds__(256) void rescore_kernel(const T *__restrict__ rows, int64_t ld, const float *__restrict__ qn,
                                                     int k, uint32_t *__restrict__ cnt, const uint32_t *__restrict__ cand,
                                                     int cap, uint64_t *__restrict__ keys, const float *__restrict__ eps,
                                                     float *__restrict__ thr, int *__restrict__ flags,
                                                     int *__restrict__ ovf_total, int final_pass, int64_t row_base,
                                                     int64_t row_stride, float *__restrict__ out_scores,
                                                     int64_t *__restrict__ out_rows, const uint32_t *__restrict__ mask) {
    constexpr bool METRIC = false, PAGED = false;
    [[maybe_unused]] const float *const norms = nullptr, *const mcoef = nullptr;  // the metric form's arguments
    [[maybe_unused]] const int32_t *const pages = nullptr;                        // the paged form's
#include "rescore_body.inc"
}
template <typename T, int NCH, int CAP, bool MASKED>
__global__ __launch_bounds__(256) void rescore_metric_kernel(const T *__restrict__ rows, int64_t ld, const float *__restrict__ qn,
                                                            int k, uint32_t *__restrict__ cnt, const uint32_t *__restrict__ cand,
                                                            int cap, uint64_t *__restrict__ keys, float *__restrict__ thr,
                                                            int *__restrict__ flags, int *__restrict__ ovf_total, int final_pass,
                                                            int64_t row_base, int64_t row_stride, float *__restrict__ out_scores,
                                                            int64_t *__restrict__ out_rows, const uint32_t *__restrict__ mask,
                                                            const float *__restrict__ norms, const float *__restrict__ mcoef) {
    constexpr bool METRIC = true, PAGED = false;
    [[maybe_unused]] const float *const eps = nullptr;  // the cosine form's argument: thr takes no slack here
    [[maybe_unused]] const int32_t *const pages = nullptr;
#include "rescore_body.inc"
}

// The metric form's launch, for the f16 / bf16 rows the metric filter serves.  search_mfma.hip
// calls it through an extern template declaration; rescore_metric_{f16,bf16}.hip instantiate it.
template <typename T>
void launch_rescore_metric(const BatchPlan &p, const BatchWs &ws, int final_pass, hipStream_t s) {
    static_assert(sizeof(T) == 2, "the metric filter serves f16 / bf16 rows");
    const bool ok = with_nch<16, T>(p.nch, [&](auto nch) {
        with_topk_cap(topk_cap(p.k), [&](auto cap) {
            auto launch = [&](auto masked) {
                hipLaunchKernelGGL((rescore_metric_kernel<T, decltype(nch)::value, decltype(cap)::value, decltype(masked)::value>),
                                   dim3(p.nq), dim3(256), 0, s, (const T *)p.rows, p.ld, ws.qn, p.k, ws.cnt, ws.cand, ws.cap, ws.keys,
                                   ws.thr, ws.flags, ws.ovf, final_pass, p.row_base, p.row_stride, p.out_scores, p.out_rows, p.mask,
                                   p.norms, ws.mcoef);
            };
            if (p.mask != nullptr) launch(std::true_type{});
            else launch(std::false_type{});
        });
    });
    if (!ok) throw Error(RC_ERR_UNSUPPORTED, "unsupported row width");
    RC_LAUNCH_CHECK();
}

// The page-table form of both (BatchPlan::pages, a named namespace's batched search): one kernel,
// METRIC a template parameter (a new symbol either way).  `rows` and `norms` are the pool's, `cand`
// holds positions, `mask` is over positions and the keys carry positions, so RC_EMIT_KEY yields
// row_base + p·row_stride as the paged scan's merge does; eps is unused under METRIC, norms and
// mcoef without it.  Instantiated in rescore_paged_{f16,bf16}.hip.
template <typename T, int NCH, int CAP, bool MASKED, bool METRIC>
__global__ __launch_bounds__(256) void rescore_paged_kernel(const T *__restrict__ rows, int64_t ld, const float *__restrict__ qn,
                                                           int k, uint32_t *__restrict__ cnt, const uint32_t *__restrict__ cand,
                                                           int cap, uint64_t *__restrict__ keys, const float *__restrict__ eps,
                                                           float *__restrict__ thr, int *__restrict__ flags,
                                                           int *__restrict__ ovf_total, int final_pass, int64_t row_base,
                                                           int64_t row_stride, float *__restrict__ out_scores,
                                                           int64_t *__restrict__ out_rows, const uint32_t *__restrict__ mask,
                                                           const float *__restrict__ norms, const float *__restrict__ mcoef,
                                                           const int32_t *__restrict__ pages) {
    constexpr bool PAGED = true;
#include "rescore_body.inc"
}

template <typename T>
void launch_rescore_paged(const BatchPlan &p, const BatchWs &ws, int final_pass, hipStream_t s) {
    static_assert(sizeof(T) == 2, "the paged batched search serves f16 / bf16 rows");
    const bool ok = with_nch<16, T>(p.nch, [&](auto nch) {
        with_topk_cap(topk_cap(p.k), [&](auto cap) {
            auto launch = [&](auto masked, auto metric) {
                hipLaunchKernelGGL((rescore_paged_kernel<T, decltype(nch)::value, decltype(cap)::value, decltype(masked)::value,
                                                         decltype(metric)::value>),
                                   dim3(p.nq), dim3(256), 0, s, (const T *)p.rows, p.ld, ws.qn, p.k, ws.cnt, ws.cand, ws.cap, ws.keys,
                                   ws.eps, ws.thr, ws.flags, ws.ovf, final_pass, p.row_base, p.row_stride, p.out_scores, p.out_rows,
                                   p.mask, p.norms, ws.mcoef, p.pages);
            };
            auto with_mask = [&](auto metric) {
                if (p.mask != nullptr) launch(std::true_type{}, metric);
                else launch(std::false_type{}, metric);
            };
            if (p.metric != RC_METRIC_COSINE) with_mask(std::true_type{});
            else with_mask(std::false_type{});
        });
    });
    if (!ok) throw Error(RC_ERR_UNSUPPORTED, "unsupported row width");
    RC_LAUNCH_CHECK();
}

}  // namespace rc
