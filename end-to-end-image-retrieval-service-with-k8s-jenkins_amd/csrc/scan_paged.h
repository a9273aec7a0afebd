// scan_paged.h — the page-table form of the streaming scan (scan.h's scan_rows_q / scan_rows):
// a namespace's vectors are dense in POSITION space [0, n_pos) of a shard, and position p lives
// at local row pages[p / RC_PAGE_ROWS] * RC_PAGE_ROWS + p % RC_PAGE_ROWS of the shard's rows (the
// pool every named namespace shares; DESIGN.md, "Namespaces").  Included only by
// scan_paged_{f32,f16,bf16,f8}.hip (cosine) and scan_paged_metric_{f32,f16,bf16,f8}.hip
// (dotproduct / euclidean), which instantiate launch_scan_paged<T> / launch_scan_paged_metric<T>
// for one storage dtype each: eight more translation units that compile in parallel, and
// scan.h's kernels keep their code.
//
// A sibling of scan_rows_q, not a PAGED parameter on it: the contiguous scan's f32 / 512-wide
// form sits at its 128-VGPR cap and every one of its kernels is pinned by the search paths'
// bit-identity tests; the copy keeps them out of reach.  What the two share stays shared:
// RC_ROW_FMA16, sum16, metric_score, WaveTopK, RC_FOLD_WAVE_LISTS, the key and the block shape.
// Everything is indexed by position but the row (and norm) address, so a block's partial list
// holds the keys the contiguous scan would give a dense index of the same vectors in position
// order, and the merges after it are the existing ones.
#pragma once

#include "paged.h"
#include "scan.h"

namespace rc {

static_assert(RC_PAGE_ROWS % 32 == 0 && RC_PAGE_ROWS % (16 * 4) == 0,
              "a page is whole mask words and whole block iterations (16 SCAN_U rows, SCAN_U <= 4)");

// scan_rows_q over positions [0, n_pos).  A wave's 4 SCAN_U positions start at a multiple of
// 4 SCAN_U (r0 is one of 32), a divisor of RC_PAGE_ROWS: they lie in one page, whose number is one
// wave-uniform word per iteration, loaded one iteration ahead of its use (as the masked scan's
// mask word).  Positions at or past r1 in the wave's group are inside the same page, hence
// inside the rows (the host checks every page against the capacity): their stale bytes are
// loaded, never pushed — no clamp, the page may belong to no other position of this block.
// MASKED: the bitmap is over positions, word g >> 5 (8 aligned words per page).
template <typename T, int NCH, int QB, int CAP, bool MASKED, bool METRIC>
__device__ __forceinline__ void scan_rows_q_paged(const T *__restrict__ rows, int64_t ld, int64_t n_pos, int64_t rows_per_block,
                                                  const int32_t *__restrict__ pages,
                                                  const float (&q)[QB][RowShape<T, NCH>::CPL][RowShape<T, NCH>::EPC], int q0,
                                                  int nq_total, int k, uint64_t *__restrict__ partial,
                                                  const uint32_t *__restrict__ mask, const float *__restrict__ norms,
                                                  MetricCoef mc) {
    static_assert(!METRIC || QB == 1, "the metric scans take one query per pass");
    constexpr int EPC = RowShape<T, NCH>::EPC;
    constexpr int CPL = RowShape<T, NCH>::CPL;
    constexpr int SCAN_U = scan_u<T, QB>();
    static_assert(RowShape<T, NCH>::WHOLE, "16 lanes x CPL chunks must cover the row");
    static_assert(RC_PAGE_ROWS % (16 * SCAN_U) == 0, "an iteration never straddles two pages");
    __shared__ uint64_t lds[4][QB][CAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rg = lane >> 4;

    WaveTopK<CAP> tk[QB];
    static_for<QB>([&](auto bc) { tk[bc.value].init(as_lds(&lds[wave][bc.value][0]), k); });

    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(n_pos, r0 + rows_per_block);
    const uint4 *base4 = reinterpret_cast<const uint4 *>(rows);
    const int64_t ld4 = ld / EPC;  // row stride in 16-B chunks

    static_assert(!MASKED || 32 % (4 * SCAN_U) == 0, "the masked scan reads a wave's row bits from one mask word");
    [[maybe_unused]] constexpr uint32_t MBITS = (1u << (4 * SCAN_U)) - 1u;
    [[maybe_unused]] uint32_t mword = 0;  // MASKED: the mask word of this wave's next iteration
    int32_t pnext = 0;                    // the page number of this wave's next iteration
    {
        const int64_t g0 = r0 + wave * 4 * SCAN_U;
        if (g0 < r1) {  // g0 < r1 <= n_pos: inside the table's ceil(n_pos / RC_PAGE_ROWS) entries and the bitmap's words
            pnext = pages[g0 / RC_PAGE_ROWS];
            if constexpr (MASKED) mword = mask[g0 >> 5];
        }
    }
    for (int64_t g = r0 + wave * 4 * SCAN_U; g < r1; g += 16 * SCAN_U) {
        const int64_t page = __builtin_amdgcn_readfirstlane(pnext);
        [[maybe_unused]] uint32_t mbyte = MBITS;  // MASKED: bit j = position g + j is eligible
        const int64_t gn = g + 16 * SCAN_U;
        if (gn < r1) pnext = pages[gn / RC_PAGE_ROWS];
        if constexpr (MASKED) {
            mbyte = ((uint32_t)__builtin_amdgcn_readfirstlane((int)mword) >> (uint32_t)(g & 31)) & MBITS;
            if (gn < r1) mword = mask[gn >> 5];
            if (mbyte == 0u) continue;  // wave-uniform: none of the wave's positions is eligible, no row is loaded
        }
        // local row of position g: the wave's 4 SCAN_U positions follow it inside the page
        const int64_t lrow = page * RC_PAGE_ROWS + (g & (RC_PAGE_ROWS - 1));
        [[maybe_unused]] float nrm[SCAN_U];  // METRIC: the norms of this lane's rows
        if constexpr (METRIC) {
#pragma unroll
            for (int u = 0; u < SCAN_U; ++u) nrm[u] = norms[lrow + u * 4 + rg];
        }
        uint4 x[SCAN_U][CPL];
#pragma unroll
        for (int u = 0; u < SCAN_U; ++u) {
            const int64_t rr = lrow + u * 4 + rg;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const u32x4_nt v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_nt *>(base4 + rr * ld4 + sub + 16 * i));
                x[u][i] = make_uint4(v.x, v.y, v.z, v.w);
            }
        }
#pragma unroll
        for (int u = 0; u < SCAN_U; ++u) {
            const int64_t r = g + u * 4 + rg;  // the key carries the position
            float acc[QB];
            RC_ROW_FMA16(T, QB, CPL, EPC, x[u], q, acc);
            static_for<QB>([&](auto bc) {
                constexpr int b = bc.value;
                float s = sum16(acc[b]);
                if constexpr (METRIC) s = metric_score(mc, s, nrm[u]);
                tk[b].reserve(4);
                if constexpr (MASKED)
                    tk[b].push(sub == 0 && r < r1 && ((mbyte >> (u * 4 + rg)) & 1u) != 0u, make_key(s, (uint32_t)r));
                else
                    tk[b].push(sub == 0 && r < r1, make_key(s, (uint32_t)r));
            });
        }
    }

    // per-wave final selection, then wave 0 merges the other three waves' lists (as scan_rows_q)
    static_for<QB>([&](auto bc) { tk[bc.value].compact(); });
    __syncthreads();
    if (wave == 0) {
        static_for<QB>([&](auto bc) {
            constexpr int b = bc.value;
            const int qi = q0 + b;
            RC_FOLD_WAVE_LISTS(&lds[w][b][0], tk[b], k, lane);
            uint64_t *dst = partial + ((int64_t)blockIdx.x * nq_total + qi) * k;
            for (int j = lane; j < k; j += 64) dst[j] = tk[b].buf[j];
        });
    }
}

// One pass of the paged scan: QB raw queries from q0 on, each normalised by every wave for itself
// (scan_rows' raw-query branch: wave_inv_norm / RC_UNIT_ELEM, the same bits), then the rows.
template <typename T, int NCH, int QB, int CAP, bool MASKED, bool METRIC>
__global__ __launch_bounds__(256, (scan_min_waves<T, NCH, QB, CAP>())) void scan_topk_paged_kernel(
    const T *__restrict__ rows, const float *__restrict__ norms, int64_t ld, int64_t n_pos, int64_t rows_per_block,
    const int32_t *__restrict__ pages, int q0, int nq_total, int k, uint64_t *__restrict__ partial,
    const float *__restrict__ qraw, int dim, int nq_real, const uint32_t *__restrict__ mask, int metric) {
    constexpr int EPC = RowShape<T, NCH>::EPC;
    constexpr int CPL = RowShape<T, NCH>::CPL;
    const int lane = threadIdx.x & 63, sub = lane & 15;
    float q[QB][CPL][EPC];
    [[maybe_unused]] MetricCoef mc{};
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        const bool valid = q0 + b < nq_real;
        const float *src = qraw + (int64_t)(valid ? q0 + b : 0) * dim;
        float inv;
        if constexpr (METRIC) {
            const float ss = wave_sum_sq(src, dim, lane, valid);
            inv = inv_norm_of(ss);
            mc = metric_coef(metric, ss);
        } else {
            inv = wave_inv_norm(src, dim, lane, valid);
        }
#pragma unroll
        for (int i = 0; i < CPL; ++i)
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const int c = (sub + 16 * i) * EPC + e;
                q[b][i][e] = RC_UNIT_ELEM(src, c, dim, inv, valid);
                if constexpr (sizeof(T) == 1) q[b][i][e] *= query_unscale<T>();  // exact: a power of two
            }
    }
    scan_rows_q_paged<T, NCH, QB, CAP, MASKED, METRIC>(rows, ld, n_pos, rows_per_block, pages, q, q0, nq_total, k, partial, mask,
                                                       norms, mc);
}

// The exact fallback of the paged batched search (search_mfma_paged.hip; f16 / bf16 rows, the
// dtypes that search serves), as scan_topk_kernel's fallback branch and scan_topk_metric_fallback_kernel:
// block (b, y) scans its position range for the queries y, y + gridDim.y, ... whose candidate list
// overflowed (flags: a block-uniform early exit for the others), one query per pass, each
// normalised from the raw queries exactly as the kernel above does (so the keys are the paged
// scan's, bit for bit); partial is [nblk][nq_total][k], merged by the existing merge under the flags.
template <typename T, int NCH, int CAP, bool MASKED, bool METRIC>
__global__ __launch_bounds__(256) void scan_topk_paged_fallback_kernel(
    const T *__restrict__ rows, const float *__restrict__ norms, int64_t ld, int64_t n_pos, int64_t rows_per_block,
    const int32_t *__restrict__ pages, int nq_total, int k, uint64_t *__restrict__ partial, const int *__restrict__ flags,
    const float *__restrict__ qraw, int dim, const uint32_t *__restrict__ mask, int metric) {
    constexpr int EPC = RowShape<T, NCH>::EPC;
    constexpr int CPL = RowShape<T, NCH>::CPL;
    const int lane = threadIdx.x & 63, sub = lane & 15;
    for (int qf = blockIdx.y; qf < nq_total; qf += gridDim.y) {
        if (!flags[qf]) continue;  // block-uniform
        float q[1][CPL][EPC];
        [[maybe_unused]] MetricCoef mc{};
        const float *src = qraw + (int64_t)qf * dim;
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
            for (int e = 0; e < EPC; ++e) q[0][i][e] = RC_UNIT_ELEM(src, (sub + 16 * i) * EPC + e, dim, inv, true);
        scan_rows_q_paged<T, NCH, 1, CAP, MASKED, METRIC>(rows, ld, n_pos, rows_per_block, pages, q, qf, nq_total, k, partial, mask,
                                                          norms, mc);
        __syncthreads();  // the next query reuses the LDS lists
    }
}

// the fallback launch of both launchers below: grid.y strides over the queries
template <typename T, bool METRIC>
void launch_scan_paged_fallback(const PagedScanArgs &p) {
    const ScanArgs &a = p.scan;
    if constexpr (sizeof(T) == 2) {
        if (a.qb != 1 || a.nq_real != a.nq_total || (METRIC && a.norms == nullptr))
            throw Error(RC_ERR_INVALID, "internal: the paged fallback scan takes unpadded raw queries, one per pass");
        const dim3 grid(a.nblk, a.grid_y);
        const bool ok = with_nch<16, T>(a.nch, [&](auto nch) {
            with_topk_cap(topk_cap(a.k), [&](auto cap) {
                constexpr int NCH = decltype(nch)::value, CAP = decltype(cap)::value;
                auto launch = [&](auto masked) {
                    hipLaunchKernelGGL((scan_topk_paged_fallback_kernel<T, NCH, CAP, decltype(masked)::value, METRIC>), grid,
                                       dim3(256), 0, a.stream, (const T *)a.rows, a.norms, a.ld, a.n_rows, a.rows_per_block, p.pages,
                                       a.nq_total, a.k, a.partial, a.flags, a.qraw, a.dim, a.mask, a.metric);
                };
                if (a.mask != nullptr) launch(std::true_type{});
                else launch(std::false_type{});
            });
        });
        if (!ok) throw Error(RC_ERR_UNSUPPORTED, "unsupported row width");
        RC_LAUNCH_CHECK();
    } else {
        throw Error(RC_ERR_INVALID, "internal: the paged fallback scan serves f16 / bf16 rows");
    }
}

template <typename T, int NCH, int QB, int CAP, bool MASKED, bool METRIC>
void launch_scan_paged_one(const PagedScanArgs &p) {
    const ScanArgs &a = p.scan;
    hipLaunchKernelGGL((scan_topk_paged_kernel<T, NCH, QB, CAP, MASKED, METRIC>), dim3(a.nblk), dim3(256), 0, a.stream,
                       (const T *)a.rows, a.norms, a.ld, a.n_rows, a.rows_per_block, p.pages, a.q0, a.nq_total, a.k, a.partial,
                       a.qraw, a.dim, a.nq_real, a.mask, a.metric);
}

inline void check_paged_args(const PagedScanArgs &p) {
    if (p.pages == nullptr || p.scan.qraw == nullptr)
        throw Error(RC_ERR_INVALID, "internal: a paged scan takes a page table and raw queries");
}

// The instantiations of the contiguous scan (launch_scan_qb): multi-query passes up to CAP 256,
// the masked ones at CAP 128 only (scan_max_qb).
template <typename T, int NCH, int QB>
void launch_scan_paged_qb(const PagedScanArgs &p) {
    const int k = p.scan.k;
    if (p.scan.mask != nullptr) {
        const bool ok = with_topk_cap<(QB == 1 ? 512 : 128)>(
            topk_cap(k), [&](auto cap) { launch_scan_paged_one<T, NCH, QB, decltype(cap)::value, true, false>(p); });
        if (!ok) throw Error(RC_ERR_UNSUPPORTED, "masked multi-query pass needs k <= 64");
    } else {
        const bool ok = with_topk_cap<(QB == 1 ? 512 : 256)>(
            topk_cap(k), [&](auto cap) { launch_scan_paged_one<T, NCH, QB, decltype(cap)::value, false, false>(p); });
        if (!ok) throw Error(RC_ERR_UNSUPPORTED, "multi-query pass needs k <= 128");
    }
    RC_LAUNCH_CHECK();
}

template <typename T>
void launch_scan_paged(const PagedScanArgs &p) {
    check_paged_args(p);
    const ScanArgs &a = p.scan;
    if (a.flags != nullptr) return launch_scan_paged_fallback<T, false>(p);  // the paged batched search's exact fallback
    const bool ok = with_nch<16, T>(a.nch, [&](auto nch) {
        constexpr int NCH = decltype(nch)::value;
        if constexpr (NCH <= 2) {  // queries per pass: scan_max_qb's register budget
            if (a.qb == 4) return launch_scan_paged_qb<T, NCH, 4>(p);
        }
        if constexpr (NCH <= 4) {
            if (a.qb == 2) return launch_scan_paged_qb<T, NCH, 2>(p);
        }
        if (a.qb == 1) return launch_scan_paged_qb<T, NCH, 1>(p);
        throw Error(RC_ERR_INVALID, "internal: no scan instantiation for this queries-per-pass");
    });
    if (!ok) throw Error(RC_ERR_UNSUPPORTED, "unsupported row width");
}

template <typename T>
void launch_scan_paged_metric(const PagedScanArgs &p) {
    check_paged_args(p);
    const ScanArgs &a = p.scan;
    if (a.flags != nullptr) return launch_scan_paged_fallback<T, true>(p);
    if (a.norms == nullptr || a.qb != 1) throw Error(RC_ERR_INVALID, "internal: a metric scan takes one query per pass and the norms");
    const bool ok = with_nch<16, T>(a.nch, [&](auto nch) {
        with_topk_cap(topk_cap(a.k), [&](auto cap) {
            constexpr int NCH = decltype(nch)::value, CAP = decltype(cap)::value;
            if (a.mask != nullptr) launch_scan_paged_one<T, NCH, 1, CAP, true, true>(p);
            else launch_scan_paged_one<T, NCH, 1, CAP, false, true>(p);
        });
    });
    if (!ok) throw Error(RC_ERR_UNSUPPORTED, "unsupported row width");
    RC_LAUNCH_CHECK();
}

}  // namespace rc
