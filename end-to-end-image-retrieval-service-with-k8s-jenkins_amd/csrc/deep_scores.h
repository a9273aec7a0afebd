// deep_scores.h — the score pass of the deep top-k (deep.h): scan_rows_q's and scan_rows_q_paged's
// row loop without the top-k and without a mask.  Included only by deep_scores_{f32,f16,bf16,f8}.hip,
// which instantiate launch_deep_scores<T> for one storage dtype each (contiguous and page-table
// form, cosine and METRIC form), so the scan units keep their kernels.
//
// What it shares with the scans is what carries their bits: the query set-up of scan_rows' raw
// branch (wave_sum_sq / inv_norm_of / RC_UNIT_ELEM, metric_coef, the f8 unscale), RC_ROW_FMA16,
// sum16 and metric_score.  A row's score therefore is the f32 the scan's key is made of.
#pragma once

#include "deep.h"
#include "scan.h"
#include "scan_paged.h"

namespace rc {

// Block (b, y): rows (PAGED: positions) [b * rows_per_block, ...) of query y.  rows_per_block is a
// multiple of 32, so a wave's 4 SCAN_U rows start at a multiple of 4 SCAN_U and (PAGED) lie in
// one page (scan_paged.h's static_asserts).  Lane sub == 0 of a row's 16 lanes stores its score.
template <typename T, int NCH, bool PAGED, bool METRIC>
__global__ __launch_bounds__(256) void scan_scores_kernel(const T *__restrict__ rows, const float *__restrict__ norms, int64_t ld,
                                                         int64_t n_rows, int64_t rows_per_block,
                                                         const int32_t *__restrict__ pages, const float *__restrict__ qraw,
                                                         int dim, int metric, float *__restrict__ ws_scores) {
    constexpr int EPC = RowShape<T, NCH>::EPC;
    constexpr int CPL = RowShape<T, NCH>::CPL;
    constexpr int SCAN_U = scan_u<T, 1>();
    static_assert(RowShape<T, NCH>::WHOLE, "16 lanes x CPL chunks must cover the row");
    static_assert(RC_PAGE_ROWS % (16 * SCAN_U) == 0, "an iteration never straddles two pages");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rg = lane >> 4;

    // the query, normalised by every wave for itself (scan_rows' raw-query branch: the same bits)
    float q[1][CPL][EPC];
    [[maybe_unused]] MetricCoef mc{};
    {
        const float *src = qraw + (int64_t)blockIdx.y * dim;
        float inv;
        if constexpr (METRIC) {
            const float ss = wave_sum_sq(src, dim, lane, true);
            inv = inv_norm_of(ss);
            mc = metric_coef(metric, ss);
        } else {
            inv = wave_inv_norm(src, dim, lane, true);
        }
#pragma unroll
        for (int i = 0; i < CPL; ++i)
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const int c = (sub + 16 * i) * EPC + e;
                q[0][i][e] = RC_UNIT_ELEM(src, c, dim, inv, true);
                if constexpr (sizeof(T) == 1) q[0][i][e] *= query_unscale<T>();  // exact: a power of two
            }
    }

    float *__restrict__ dst = ws_scores + (int64_t)blockIdx.y * n_rows;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(n_rows, r0 + rows_per_block);
    const uint4 *base4 = reinterpret_cast<const uint4 *>(rows);
    const int64_t ld4 = ld / EPC;  // row stride in 16-B chunks

    [[maybe_unused]] int32_t pnext = 0;  // PAGED: the page number of this wave's next iteration
    if constexpr (PAGED) {
        const int64_t g0 = r0 + wave * 4 * SCAN_U;
        if (g0 < r1) pnext = pages[g0 / RC_PAGE_ROWS];  // g0 < n_rows: inside the table's ceil(n_rows / RC_PAGE_ROWS) entries
    }
    for (int64_t g = r0 + wave * 4 * SCAN_U; g < r1; g += 16 * SCAN_U) {
        // the local row of the iteration's first row; PAGED: the rest follow it inside the page
        // (rows past r1 there are stale bytes inside the rows, loaded and never stored)
        int64_t lrow = g;
        if constexpr (PAGED) {
            const int64_t page = __builtin_amdgcn_readfirstlane(pnext);
            const int64_t gn = g + 16 * SCAN_U;
            if (gn < r1) pnext = pages[gn / RC_PAGE_ROWS];
            lrow = page * RC_PAGE_ROWS + (g & (RC_PAGE_ROWS - 1));
        }
        int64_t rr[SCAN_U];
#pragma unroll
        for (int u = 0; u < SCAN_U; ++u) {
            const int64_t r = g + u * 4 + rg;
            if constexpr (PAGED) rr[u] = lrow + u * 4 + rg;
            else rr[u] = r < r1 ? r : r0;  // clamp to a valid row (r0 < r1 <= n_rows); the score is not stored
        }
        [[maybe_unused]] float nrm[SCAN_U];  // METRIC: the norms of this lane's rows
        if constexpr (METRIC) {
#pragma unroll
            for (int u = 0; u < SCAN_U; ++u) nrm[u] = norms[rr[u]];
        }
        uint4 x[SCAN_U][CPL];
#pragma unroll
        for (int u = 0; u < SCAN_U; ++u) {
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                // nontemporal: the rows stream through once, as in the scan
                const u32x4_nt v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_nt *>(base4 + rr[u] * ld4 + sub + 16 * i));
                x[u][i] = make_uint4(v.x, v.y, v.z, v.w);
            }
        }
#pragma unroll
        for (int u = 0; u < SCAN_U; ++u) {
            const int64_t r = g + u * 4 + rg;
            float acc[1];
            RC_ROW_FMA16(T, 1, CPL, EPC, x[u], q, acc);
            float s = sum16(acc[0]);
            if constexpr (METRIC) s = metric_score(mc, s, nrm[u]);
            if (sub == 0 && r < r1) dst[r] = s;
        }
    }
}

template <typename T>
void launch_deep_scores(const DeepScoreArgs &a) {
    if (a.nq <= 0 || a.n_rows <= 0) return;
    if (a.rows_per_block <= 0 || a.rows_per_block % 32 != 0 || (int64_t)a.nblk * a.rows_per_block < a.n_rows)
        throw Error(RC_ERR_INVALID, "internal: the score pass takes blocks of whole 32-row groups covering the rows");
    const bool metric = a.metric != RC_METRIC_COSINE;
    if (metric && a.norms == nullptr) throw Error(RC_ERR_INVALID, "internal: a metric score pass reads the norms");
    const dim3 grid(a.nblk, a.nq);
    const bool ok = with_nch<16, T>(a.nch, [&](auto nch) {
        constexpr int NCH = decltype(nch)::value;
        auto launch = [&](auto paged, auto met) {
            hipLaunchKernelGGL((scan_scores_kernel<T, NCH, decltype(paged)::value, decltype(met)::value>), grid, dim3(256), 0,
                               a.stream, (const T *)a.rows, a.norms, a.ld, a.n_rows, a.rows_per_block, a.pages, a.queries, a.dim,
                               a.metric, a.scores);
        };
        if (a.pages != nullptr) {
            if (metric) launch(std::true_type{}, std::true_type{});
            else launch(std::true_type{}, std::false_type{});
        } else {
            if (metric) launch(std::false_type{}, std::true_type{});
            else launch(std::false_type{}, std::false_type{});
        }
    });
    if (!ok) throw Error(RC_ERR_UNSUPPORTED, "unsupported row width");
    RC_LAUNCH_CHECK();
}

}  // namespace rc
