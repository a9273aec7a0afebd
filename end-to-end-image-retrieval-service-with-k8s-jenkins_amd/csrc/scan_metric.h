// scan_metric.h — the scan and the one-launch query under a non-cosine metric (dotproduct,
// euclidean: rc_index_set_metric): kernels over scan.h's METRIC device functions and their launch
// chains.  Included only by scan_metric_{f32,f16,bf16,f8}.hip, which instantiate
// launch_scan_metric<T> / launch_query1_metric_scan<T> for one storage dtype each: four more
// translation units that compile in parallel, and the cosine units keep their kernels.
#pragma once

#include "scan.h"

namespace rc {

// scan_topk_kernel / scan_topk_masked_kernel with the metric's score in the top-k keys: one raw
// query (q0 of nq_total) per pass; the fallback mode is the kernel below this one.  One
// code path for both metrics: `metric` only picks the per-query constants (metric_coef).  The
// f32 / 512-wide form keeps scan_min_waves' 128-VGPR cap: it holds it without scratch.
template <typename T, int NCH, int CAP, bool MASKED>
__global__ __launch_bounds__(256, (scan_min_waves<T, NCH, 1, CAP>())) void scan_topk_metric_kernel(
    const T *__restrict__ rows, const float *__restrict__ norms, int64_t ld, int64_t n_rows, int64_t rows_per_block, int q0,
    int nq_total, int k, uint64_t *__restrict__ partial, const float *__restrict__ qraw, int dim, int nq_real,
    const uint32_t *__restrict__ mask, int metric) {
    scan_rows<T, NCH, 1, CAP, MASKED, true>(rows, ld, n_rows, rows_per_block, nullptr, q0, nq_total, k, partial, qraw, dim, nq_real,
                                            mask, norms, metric);
}

// The exact fallback of the metric batched search (RC_FILTER_METRIC; f16 / bf16 rows, the dtypes
// that search serves): as scan_topk_kernel's fallback branch, block (b, y) scans its row range for
// the queries y, y + gridDim.y, ... whose candidate list overflowed (flags), each normalised from
// the raw queries as every metric scan does; partial is [nblk][nq_total][k].  A kernel of its own:
// scan_topk_metric_kernel keeps its arguments and its code.
template <typename T, int NCH, int CAP, bool MASKED>
__global__ __launch_bounds__(256, (scan_min_waves<T, NCH, 1, CAP>())) void scan_topk_metric_fallback_kernel(
    const T *__restrict__ rows, const float *__restrict__ norms, int64_t ld, int64_t n_rows, int64_t rows_per_block, int nq_total,
    int k, uint64_t *__restrict__ partial, const int *__restrict__ flags, const float *__restrict__ qraw, int dim,
    const uint32_t *__restrict__ mask, int metric) {
    for (int qf = blockIdx.y; qf < nq_total; qf += gridDim.y)
        if (flags[qf]) {  // block-uniform
            scan_rows<T, NCH, 1, CAP, MASKED, true>(rows, ld, n_rows, rows_per_block, nullptr, qf, nq_total, k, partial, qraw, dim,
                                                    nq_total, mask, norms, metric);
            __syncthreads();  // the next query reuses the LDS lists
        }
}

template <typename T>
void launch_scan_metric(const ScanArgs &a) {
    if (a.qraw == nullptr || a.norms == nullptr || a.qb != 1)
        throw Error(RC_ERR_INVALID, "internal: a metric scan takes raw queries, one per pass, and the norms");
    if (a.flags != nullptr && (sizeof(T) != 2 || a.nq_real != a.nq_total))
        throw Error(RC_ERR_INVALID, "internal: the metric fallback scan serves f16 / bf16 rows and unpadded queries");
    const dim3 grid(a.nblk, a.flags != nullptr ? a.grid_y : 1);
    const bool ok = with_nch<16, T>(a.nch, [&](auto nch) {
        with_topk_cap(topk_cap(a.k), [&](auto cap) {
            constexpr int NCH = decltype(nch)::value, CAP = decltype(cap)::value;
            auto launch = [&](auto masked) {
                if constexpr (sizeof(T) == 2) {
                    if (a.flags != nullptr) {
                        hipLaunchKernelGGL((scan_topk_metric_fallback_kernel<T, NCH, CAP, decltype(masked)::value>), grid, dim3(256),
                                           0, a.stream, (const T *)a.rows, a.norms, a.ld, a.n_rows, a.rows_per_block, a.nq_total,
                                           a.k, a.partial, a.flags, a.qraw, a.dim, a.mask, a.metric);
                        return;
                    }
                }
                hipLaunchKernelGGL((scan_topk_metric_kernel<T, NCH, CAP, decltype(masked)::value>), grid, dim3(256), 0, a.stream,
                                   (const T *)a.rows, a.norms, a.ld, a.n_rows, a.rows_per_block, a.q0, a.nq_total, a.k, a.partial,
                                   a.qraw, a.dim, a.nq_real, a.mask, a.metric);
            };
            if (a.mask != nullptr) launch(std::true_type{});
            else launch(std::false_type{});
        });
    });
    if (!ok) throw Error(RC_ERR_UNSUPPORTED, "unsupported row width");
    RC_LAUNCH_CHECK();
}

// Phase 1 of the one-launch query under a metric; phase 2 is query1_kernel's (the keys already
// carry the final scores).
template <typename T, int NCH, int CAP>
__global__ __launch_bounds__(256) void query1_metric_kernel(const Query1Args a) {
    query1_scan<T, NCH, CAP, true>(a);
}

template <typename T>
void launch_query1_metric_scan(const Query1Args &a, hipStream_t s) {
    const bool ok = with_nch<6, T>(a.nch, [&](auto nch) {
        const bool cap_ok = with_topk_cap<256>(topk_cap(a.k), [&](auto cap) {
            hipLaunchKernelGGL((query1_metric_kernel<T, decltype(nch)::value, decltype(cap)::value>), dim3(a.nblk), dim3(256), 0, s, a);
        });
        if (!cap_ok) throw Error(RC_ERR_UNSUPPORTED, "single-query launch needs k <= 128");
    });
    if (!ok) throw Error(RC_ERR_UNSUPPORTED, "single-query launch: row width beyond 768");
    RC_LAUNCH_CHECK();
}

}  // namespace rc
