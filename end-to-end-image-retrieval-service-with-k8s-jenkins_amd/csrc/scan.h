// scan.h — the single-query streaming scan (HBM-bound GEMV + fused wavefront top-k) and the
// one-launch query of the exact cosine index: device code and launch chains.  Included only by
// scan_{f32,f16,bf16,f8}.hip, which instantiate launch_scan<T> / launch_query1<T> for one storage
// dtype each, so the four translation units compile in parallel.  The device functions' METRIC
// forms (dotproduct / euclidean scores) are instantiated by scan_metric.h's kernels, in
// scan_metric_{f32,f16,bf16,f8}.hip.
#pragma once

#include "index_common.h"

namespace rc {

// qn holds nq_total (a multiple of QB) query rows, zero beyond the caller's
// queries, so every slot is computed and stored unconditionally.
// Block = 4 waves over a contiguous row range.  Lane = (row-in-group rg = lane>>4,
// position sub = lane&15); 16-B chunk j = sub + 16 i of a row holds elements
// [j*EPC, (j+1)*EPC).  scan_u<T, QB>() row-groups are loaded before any is consumed: 2, and 4
// for single-query passes over one-byte elements, whose row group is half the bytes — the same
// bytes in flight per wave (SCAN_U x 4 rows x ld bytes) and the same x[][] registers as an f16
// row of that width.  (Multi-query passes do QB times the arithmetic per byte and keep 2: with 4
// copies of a QB = 4 body hipcc leaves the consuming loop rolled and x[][] goes to scratch.)
template <typename T, int QB>
constexpr int scan_u() { return sizeof(T) == 1 && QB == 1 ? 4 : 2; }

typedef uint32_t u32x4_nt __attribute__((ext_vector_type(4)));  // the nontemporal load's operand type

// One block's pass over its row range for the QB queries held in registers q (lane sub's
// chunks sub + 16 i): partial top-k keys of queries q0 .. q0 + QB.
// MASKED: only rows whose bit is set in `mask` (see ScanArgs) enter the top-k.  A wave's
// iteration covers the 8 rows g .. g + 7 with g = r0 + 8 wave + 32 it and r0 a multiple of 32
// (rows_per_block is), so their bits are byte (g & 31) / 8 of word g >> 5: one wave-uniform word
// per iteration, loaded one iteration ahead of its use.  (In general 4 SCAN_U rows, a divisor of
// 32: with SCAN_U = 4 the 16 rows from g = r0 + 16 wave + 64 it are half a word, and "byte"
// below reads as those 16 bits.)  A zero byte skips the iteration's row loads altogether
// (wave-uniform branch: every reserve / push stays wave-collective) — the HBM bytes a selective
// filter saves.  The per-row arithmetic is untouched, so an eligible row's
// score has the bits the unmasked scan gives it.
// METRIC (one query per pass): the key's score is metric_score(mc, cosine, norms[row]), formed
// per row before the top-k, so the list is the metric's own top-k (index_common.h has the rule).
// The iteration's norms are loaded ahead of its rows, under the rows' clamp: they return first
// and no wait for a row group reaches past it.
template <typename T, int NCH, int QB, int CAP, bool MASKED = false, bool METRIC = false>
__device__ __forceinline__ void scan_rows_q(const T *__restrict__ rows, int64_t ld, int64_t n_rows, int64_t rows_per_block,
                                            const float (&q)[QB][RowShape<T, NCH>::CPL][RowShape<T, NCH>::EPC], int q0,
                                            int nq_total, int k, uint64_t *__restrict__ partial,
                                            const uint32_t *__restrict__ mask = nullptr,
                                            const float *__restrict__ norms = nullptr, MetricCoef mc = MetricCoef{}) {
    static_assert(!METRIC || QB == 1, "the metric scans take one query per pass");
    constexpr int EPC = RowShape<T, NCH>::EPC;
    constexpr int CPL = RowShape<T, NCH>::CPL;
    constexpr int SCAN_U = scan_u<T, QB>();
    static_assert(RowShape<T, NCH>::WHOLE, "16 lanes x CPL chunks must cover the row");
    __shared__ uint64_t lds[4][QB][CAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rg = lane >> 4;

    WaveTopK<CAP> tk[QB];
    static_for<QB>([&](auto bc) { tk[bc.value].init(as_lds(&lds[wave][bc.value][0]), k); });

    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(n_rows, r0 + rows_per_block);
    const uint4 *base4 = reinterpret_cast<const uint4 *>(rows);
    const int64_t ld4 = ld / EPC;  // row stride in 16-B chunks

    // a wave's 4 SCAN_U rows start at a multiple of 4 SCAN_U (r0 is one of 32): inside one word
    static_assert(!MASKED || 32 % (4 * SCAN_U) == 0, "the masked scan reads a wave's row bits from one mask word");
    [[maybe_unused]] constexpr uint32_t MBITS = (1u << (4 * SCAN_U)) - 1u;
    [[maybe_unused]] uint32_t mword = 0;  // MASKED: the mask word of this wave's next iteration
    if constexpr (MASKED) {
        const int64_t g0 = r0 + wave * 4 * SCAN_U;
        if (g0 < r1) mword = mask[g0 >> 5];  // g0 < r1 <= n_rows: inside the bitmap's ceil(n_rows / 32) words
    }
    for (int64_t g = r0 + wave * 4 * SCAN_U; g < r1; g += 16 * SCAN_U) {
        [[maybe_unused]] uint32_t mbyte = MBITS;  // MASKED: bit j = row g + j is eligible
        if constexpr (MASKED) {
            mbyte = ((uint32_t)__builtin_amdgcn_readfirstlane((int)mword) >> (uint32_t)(g & 31)) & MBITS;
            const int64_t gn = g + 16 * SCAN_U;
            if (gn < r1) mword = mask[gn >> 5];
            if (mbyte == 0u) continue;  // wave-uniform: none of the wave's rows is eligible, no row is loaded
        }
        [[maybe_unused]] float nrm[SCAN_U];  // METRIC: the norms of this lane's rows
        if constexpr (METRIC) {
#pragma unroll
            for (int u = 0; u < SCAN_U; ++u) {
                const int64_t r = g + u * 4 + rg;
                nrm[u] = norms[r < r1 ? r : r0];  // r0 < r1 <= n_rows: inside the norms
            }
        }
        uint4 x[SCAN_U][CPL];
#pragma unroll
        for (int u = 0; u < SCAN_U; ++u) {
            const int64_t r = g + u * 4 + rg;
            const int64_t rr = r < r1 ? r : r0;  // clamp to a valid row; result discarded below
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                // nontemporal: the rows stream through once (scan lab, 1M x 512 f32: 6.2 -> 7.0 TB/s)
                const u32x4_nt v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_nt *>(base4 + rr * ld4 + sub + 16 * i));
                x[u][i] = make_uint4(v.x, v.y, v.z, v.w);
            }
        }
#pragma unroll
        for (int u = 0; u < SCAN_U; ++u) {
            const int64_t r = g + u * 4 + rg;
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

    // per-wave final selection, then wave 0 merges the other three waves' lists
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

// The scan kernels' query set-up: the QB queries' register chunks, either from the normalised
// rows qn or (qraw: the single-query scans) normalised here from the raw queries, every wave
// for itself (wave_inv_norm / RC_UNIT_ELEM: the bits qn would hold).
// METRIC: raw queries only (qn is not read); the same sum of squares gives the normalisation
// and the metric's per-query constants (metric_coef).
template <typename T, int NCH, int QB, int CAP, bool MASKED = false, bool METRIC = false>
__device__ __forceinline__ void scan_rows(const T *__restrict__ rows, int64_t ld, int64_t n_rows, int64_t rows_per_block,
                                          const float *__restrict__ qn, int q0, int nq_total, int k,
                                          uint64_t *__restrict__ partial, const float *__restrict__ qraw = nullptr,
                                          int dim = 0, int nq_real = 0, const uint32_t *__restrict__ mask = nullptr,
                                          const float *__restrict__ norms = nullptr, int metric = RC_METRIC_COSINE) {
    constexpr int EPC = RowShape<T, NCH>::EPC;
    constexpr int CPL = RowShape<T, NCH>::CPL;
    const int lane = threadIdx.x & 63, sub = lane & 15;
    float q[QB][CPL][EPC];
    [[maybe_unused]] MetricCoef mc{};
    if (METRIC || qraw != nullptr) {  // block-uniform
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
    } else {
#pragma unroll
        for (int b = 0; b < QB; ++b)
#pragma unroll
            for (int i = 0; i < CPL; ++i)
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    q[b][i][e] = qn[(int64_t)(q0 + b) * ld + (sub + 16 * i) * EPC + e];
                    if constexpr (sizeof(T) == 1) q[b][i][e] *= query_unscale<T>();
                }
    }
    scan_rows_q<T, NCH, QB, CAP, MASKED, METRIC>(rows, ld, n_rows, rows_per_block, q, q0, nq_total, k, partial, mask, norms, mc);
}

// f32 rows of 512 (config 3): 131 VGPRs by default = 3 waves per SIMD; capped at 128 (no spill)
// the CU holds 4 blocks and a 1M-row scan runs as one round of 4 blocks per CU
template <typename T, int NCH, int QB, int CAP>
constexpr int scan_min_waves() { return (sizeof(T) == 4 && NCH == 4 && QB == 1 && CAP <= 256) ? 4 : 1; }

template <typename T, int NCH, int QB, int CAP>
__global__ __launch_bounds__(256, (scan_min_waves<T, NCH, QB, CAP>())) void scan_topk_kernel(const T *__restrict__ rows, int64_t ld, int64_t n_rows,
                                                       int64_t rows_per_block, const float *__restrict__ qn, int q0,
                                                       int nq_total, int k, uint64_t *__restrict__ partial,
                                                       const int *__restrict__ flags, const float *__restrict__ qraw,
                                                       int dim, int nq_real) {
    if (flags != nullptr) {  // exact fallback: the overflowed queries only (block-uniform branches)
        for (int qf = blockIdx.y; qf < nq_total; qf += gridDim.y)
            if (flags[qf]) {
                scan_rows<T, NCH, QB, CAP>(rows, ld, n_rows, rows_per_block, qn, qf, nq_total, k, partial);
                __syncthreads();  // the next query reuses the LDS lists
            }
        return;
    }
    scan_rows<T, NCH, QB, CAP>(rows, ld, n_rows, rows_per_block, qn, q0, nq_total, k, partial, qraw, dim, nq_real);
}

// The row-masked form of scan_topk_kernel (both of its modes).  A kernel of its own, not a
// runtime test of a null mask: the unmasked instantiations keep their code and registers (the
// f32 / 512-wide one sits at the 128-VGPR cap above).
template <typename T, int NCH, int QB, int CAP>
__global__ __launch_bounds__(256, (scan_min_waves<T, NCH, QB, CAP>())) void scan_topk_masked_kernel(
    const T *__restrict__ rows, int64_t ld, int64_t n_rows, int64_t rows_per_block, const float *__restrict__ qn, int q0,
    int nq_total, int k, uint64_t *__restrict__ partial, const int *__restrict__ flags, const float *__restrict__ qraw, int dim,
    int nq_real, const uint32_t *__restrict__ mask) {
    if (flags != nullptr) {  // exact fallback of the masked batched search
        for (int qf = blockIdx.y; qf < nq_total; qf += gridDim.y)
            if (flags[qf]) {
                scan_rows<T, NCH, QB, CAP, true>(rows, ld, n_rows, rows_per_block, qn, qf, nq_total, k, partial, nullptr, 0, 0, mask);
                __syncthreads();
            }
        return;
    }
    scan_rows<T, NCH, QB, CAP, true>(rows, ld, n_rows, rows_per_block, qn, q0, nq_total, k, partial, qraw, dim, nq_real, mask);
}

// Multi-query passes are instantiated up to CAP 256 (k <= 128), the masked ones at CAP 128 only
// (k <= 64: scan_max_qb).
template <typename T, int NCH, int QB>
void launch_scan_qb(const ScanArgs &a) {
    const dim3 grid(a.nblk, a.grid_y);
    const T *rows = (const T *)a.rows;
    if (a.mask != nullptr) {  // host-side choice of the masked instantiations
        const bool ok = with_topk_cap<(QB == 1 ? 512 : 128)>(topk_cap(a.k), [&](auto cap) {
            hipLaunchKernelGGL((scan_topk_masked_kernel<T, NCH, QB, decltype(cap)::value>), grid, dim3(256), 0, a.stream, rows,
                               a.ld, a.n_rows, a.rows_per_block, a.qn, a.q0, a.nq_total, a.k, a.partial, a.flags, a.qraw, a.dim,
                               a.nq_real, a.mask);
        });
        if (!ok) throw Error(RC_ERR_UNSUPPORTED, "masked multi-query pass needs k <= 64");
    } else {
        const bool ok = with_topk_cap<(QB == 1 ? 512 : 256)>(topk_cap(a.k), [&](auto cap) {
            hipLaunchKernelGGL((scan_topk_kernel<T, NCH, QB, decltype(cap)::value>), grid, dim3(256), 0, a.stream, rows, a.ld,
                               a.n_rows, a.rows_per_block, a.qn, a.q0, a.nq_total, a.k, a.partial, a.flags, a.qraw, a.dim,
                               a.nq_real);
        });
        if (!ok) throw Error(RC_ERR_UNSUPPORTED, "multi-query pass needs k <= 128");
    }
    RC_LAUNCH_CHECK();
}

template <typename T>
void launch_scan(const ScanArgs &a) {
    if (a.metric != RC_METRIC_COSINE) return launch_scan_metric<T>(a);  // the metric kernels' own translation units
    const bool ok = with_nch<16, T>(a.nch, [&](auto nch) {
        constexpr int NCH = decltype(nch)::value;
        if constexpr (NCH <= 2) {  // queries per pass: scan_max_qb's register budget
            if (a.qb == 4) return launch_scan_qb<T, NCH, 4>(a);
        }
        if constexpr (NCH <= 4) {
            if (a.qb == 2) return launch_scan_qb<T, NCH, 2>(a);
        }
        if (a.qb == 1) return launch_scan_qb<T, NCH, 1>(a);
        throw Error(RC_ERR_INVALID, "internal: no scan instantiation for this queries-per-pass");
    });
    if (!ok) throw Error(RC_ERR_UNSUPPORTED, "unsupported row width");
}

// rc_sharded_query_host's single-query launch pair (see Query1Args).  Every wave normalises the
// query with wave_inv_norm / RC_UNIT_ELEM, as the multi-kernel path's scan does (same lane partition
// of the sum of squares, same wave_sum, same products), so scores are bit-identical to it; the
// top-k of a total order does not depend on how rows are split over blocks.  PHASE 1: the scan
// blocks, each writing its partial list; PHASE 2: one block merges them (the kernel boundary
// orders the lists: a one-launch form with a last-block ticket behind device-scope fences
// measured 5.6 us slower per 10k-row call, round 4) and gathers the values.
template <typename T, int NCH, int CAP, bool METRIC = false>
__device__ __forceinline__ void query1_scan(const Query1Args &a) {
    constexpr int EPC = RowShape<T, NCH>::EPC;
    constexpr int CPL = RowShape<T, NCH>::CPL;
    const int lane = threadIdx.x & 63, sub = lane & 15;
    // the kernarg segment may sit in host memory: one round of independent loads into LDS
    // (no branches), then every read is local
    __shared__ float qs[QUERY1_MAX_DIM];
    {
        constexpr int PER = QUERY1_MAX_DIM / 256;
        float v[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) v[i] = a.q[threadIdx.x + 256 * i];
#pragma unroll
        for (int i = 0; i < PER; ++i) qs[threadIdx.x + 256 * i] = v[i];
    }
    __syncthreads();
    float inv;
    [[maybe_unused]] MetricCoef mc{};
    if constexpr (METRIC) {  // as scan_rows' metric form: one sum of squares, the same bits
        const float ss = wave_sum_sq(qs, a.dim, lane);
        inv = inv_norm_of(ss);
        mc = metric_coef(a.metric, ss);
    } else {
        inv = wave_inv_norm(qs, a.dim, lane);
    }
    float q[1][CPL][EPC];
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const int c = (sub + 16 * i) * EPC + e;
            q[0][i][e] = RC_UNIT_ELEM(qs, c, a.dim, inv, true);
            if constexpr (sizeof(T) == 1) q[0][i][e] *= query_unscale<T>();  // as scan_rows
        }
    scan_rows_q<T, NCH, 1, CAP, false, METRIC>((const T *)a.rows, a.ld, a.n_rows, a.rows_per_block, q, 0, 1, a.k, a.partial,
                                               nullptr, a.norms, mc);
}

template <typename T, int CAP>
__device__ __forceinline__ void query1_finish(const Query1Args &a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ uint64_t lds[4][CAP];
    WaveTopK<CAP> tk;
    merge_partial_lists<CAP>(a.partial, a.nblk, 1, 0, a.k, lds, tk);
    __shared__ uint64_t best[CAP];
    if (wave == 0) {
        for (int j = lane; j < a.k; j += 64) {
            const uint64_t key = tk.buf[j];
            best[j] = key;
            RC_EMIT_KEY(key, a.row_base, a.row_stride, a.out_scores[j], a.out_rows[j]);
        }
    }
    __syncthreads();
    if (a.with_values) {  // fetch_kernel's arithmetic: stored row x norm, NaN for an empty slot
        const T *rows = (const T *)a.rows;
        for (int j = wave; j < a.k; j += 4) {
            const uint64_t key = best[j];
            float *dst = a.out_values + (int64_t)j * a.dim;
            if (key == KEY_EMPTY) {
                for (int c = lane; c < a.dim; c += 64) dst[c] = __builtin_nanf("");
            } else {
                const int64_t r = key_idx(key);
                const float nrm = a.norms[r];
                if ((a.dim & 3) == 0) {  // 16-B stores: a quarter of the write transactions to host memory
                    for (int c = 4 * lane; c < a.dim; c += 256) {
                        const int64_t o = r * a.ld + c;
                        *reinterpret_cast<float4 *>(dst + c) =
                            make_float4(Elem<T>::load(rows, o) * nrm, Elem<T>::load(rows, o + 1) * nrm,
                                        Elem<T>::load(rows, o + 2) * nrm, Elem<T>::load(rows, o + 3) * nrm);
                    }
                } else {
                    for (int c = lane; c < a.dim; c += 64) dst[c] = Elem<T>::load(rows, r * a.ld + c) * nrm;
                }
            }
        }
    }
    if (a.done != nullptr) {  // completion word for a host that polls instead of synchronising
        // Every wave releases its OWN result stores to system scope (a workgroup barrier does not
        // wait for another wave's outstanding stores), then the barrier, then one lane publishes.
        // The explicit vmcnt waits stay in inline asm: hipcc may drop a fence's own wait when it
        // believes the store counter is already empty (MI355X_MICROARCH.md, compiler hazard).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __threadfence_system();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence_system();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(a.done, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

template <typename T, int NCH, int CAP, int PHASE>
__global__ __launch_bounds__(256) void query1_kernel(const Query1Args a) {
    if constexpr (PHASE == 2) query1_finish<T, CAP>(a);
    else query1_scan<T, NCH, CAP>(a);
}

// Instantiated for row widths up to 768 (QUERY1_MAX_DIM) and k <= 128.
template <typename T>
void launch_query1(const Query1Args &a, hipStream_t s) {
    const bool ok = with_nch<6, T>(a.nch, [&](auto nch) {
        const bool cap_ok = with_topk_cap<256>(topk_cap(a.k), [&](auto cap) {
            constexpr int NCH = decltype(nch)::value, CAP = decltype(cap)::value;
            if (a.metric != RC_METRIC_COSINE) {  // phase 1 under the metric; phase 2 is the same
                launch_query1_metric_scan<T>(a, s);
            } else {
                hipLaunchKernelGGL((query1_kernel<T, NCH, CAP, 1>), dim3(a.nblk), dim3(256), 0, s, a);
                RC_LAUNCH_CHECK();
            }
            hipLaunchKernelGGL((query1_kernel<T, NCH, CAP, 2>), dim3(1), dim3(256), 0, s, a);
            RC_LAUNCH_CHECK();
        });
        if (!cap_ok) throw Error(RC_ERR_UNSUPPORTED, "single-query launch needs k <= 128");
    });
    if (!ok) throw Error(RC_ERR_UNSUPPORTED, "single-query launch: row width beyond 768");
}

}  // namespace rc
