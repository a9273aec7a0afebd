// search_mfma.hip — batched exact cosine top-k on CDNA4 matrix cores
// (BASELINE config 4: 1024 queries x top-100 over a 125M x 512 fp16 shard).
//
// Replaces index.query(vector, top_k) (retriever/utils.py:62-64) for a batch of
// query vectors; the single-query path is the HBM-bound scan (scan.h).
//
// A query batch is a GEMM: S = Q · Xᵀ (queries x rows, K = ld).  S is never
// materialised.  The search runs in STAGES over growing row ranges
// [0, b1), [b1, b2), ... with b(i+1) = g · b(i):
//   filter_gemm_kernel  MFMA (f16/bf16 in, f32 acc) 256 queries x 256 rows x 64
//                       tiles; the epilogue keeps (query, row) iff
//                       s'(q,r) >= thr[q] and appends the row to the query's
//                       candidate list (atomic counter, capacity CAND_CAP);
//   rescore_kernel      per query: exact f32 score of every candidate (RC_ROW_FMA16
//                       + sum16, the single-query scan's own row score, so both paths
//                       give bit-identical scores), wavefront top-k merge with the
//                       running top-k keys, thr[q] = kth_best - eps[q].
// Why it is exact: s' uses the query rounded to the storage dtype q̂.  For a
// stored row x̂ (||x̂|| <= 1.01) |s' - s| <= ||q - q̂||·||x̂|| + two f32
// accumulation bounds (512·2^-24 each) =: eps[q] (computed per query).  The
// running kth best T of the rows seen so far is a lower bound of the final kth
// best, so any row of the final top-k has s >= T, hence s' >= T - eps: the
// filter never drops a true member.  The stage ratio g keeps the expected
// candidates per stage at ≈ k·(g-1) ≪ CAND_CAP.  A query whose candidates
// overflow CAND_CAP in some stage (adversarial / duplicate-heavy data) is
// flagged and re-run on the device through the exact scan (index.hip,
// scan_topk_kernel's fallback mode): no host synchronisation.
//
// HBM layout: rows [cap256][ld] T (capacity rounded up to 256 rows so whole
// row tiles are readable), queries q̂ [nqb*256][ld] T (zero rows past nq).
#include <algorithm>
#include <vector>

#include "filter_mfma.h"
#include "index_common.h"
#include "rescore.h"

namespace rc {

// ------------------------------------------------------ query preparation --
// One wave per query slot q < nq_pad: qn = q/||q|| (f32, the exact rescoring
// operand: wave_inv_norm / RC_UNIT_ELEM, as the scan normalises), qh = cast(qn) (the
// MFMA operand), eps = error bound of s' (see header), thr = -inf (real
// query) or +inf (padding slot: never appends).
template <typename T>
__global__ __launch_bounds__(64) void prepare_queries_kernel(const float *__restrict__ q, int nq, int dim, int64_t ld,
                                                            float *__restrict__ qn, T *__restrict__ qh,
                                                            float *__restrict__ eps, float *__restrict__ thr) {
    const int lane = threadIdx.x;
    const int qi = blockIdx.x;
    const bool valid = qi < nq;
    const float *src = q + (int64_t)(valid ? qi : 0) * dim;
    const float inv = wave_inv_norm(src, dim, lane, valid);
    float err = 0.f;
    for (int c = lane; c < ld; c += 64) {
        const float v = RC_UNIT_ELEM(src, c, dim, inv, valid);
        const T h = Elem<T>::cast(v);
        const float d = v - Elem<T>::load(&h, 0);
        err = fmaf(d, d, err);
        if (valid) qn[(int64_t)qi * ld + c] = v;
        qh[(int64_t)qi * ld + c] = h;
    }
    err = wave_sum(err);
    if (lane == 0) {
        eps[qi] = 1.01f * sqrtf(err) + 6.5e-5f;
        thr[qi] = valid ? -INFINITY : INFINITY;
    }
}

// The metric filter's preparation (RC_FILTER_METRIC under dotproduct / euclidean): qn, qh, eps
// and thr exactly as above, plus the query's metric constants mcoef[qi] = (eps, alpha, beta,
// gamma).  (alpha, beta, gamma) = metric_coef(metric, wave_sum_sq): the metric scan's own sum of
// squares (same lane partition, same butterfly) and its own rule, so the rescored keys have the
// scan's bits.  One wave per query: the sum is wave-uniform, as metric_coef's readfirstlane needs.
template <typename T>
__global__ __launch_bounds__(64) void prepare_queries_metric_kernel(const float *__restrict__ q, int nq, int dim, int64_t ld,
                                                                   int metric, float *__restrict__ qn, T *__restrict__ qh,
                                                                   float *__restrict__ eps, float *__restrict__ thr,
                                                                   float *__restrict__ mcoef) {
    const int lane = threadIdx.x;
    const int qi = blockIdx.x;
    const bool valid = qi < nq;
    const float *src = q + (int64_t)(valid ? qi : 0) * dim;
    const float ss = wave_sum_sq(src, dim, lane, valid);
    const float inv = inv_norm_of(ss);  // wave_inv_norm's value
    const MetricCoef mc = metric_coef(metric, ss);
    float err = 0.f;
    for (int c = lane; c < ld; c += 64) {
        const float v = RC_UNIT_ELEM(src, c, dim, inv, valid);
        const T h = Elem<T>::cast(v);
        const float d = v - Elem<T>::load(&h, 0);
        err = fmaf(d, d, err);
        if (valid) qn[(int64_t)qi * ld + c] = v;
        qh[(int64_t)qi * ld + c] = h;
    }
    err = wave_sum(err);
    if (lane == 0) {
        const float e = 1.01f * sqrtf(err) + 6.5e-5f;
        eps[qi] = e;
        thr[qi] = valid ? -INFINITY : INFINITY;
        mcoef[4 * qi + 0] = e;
        mcoef[4 * qi + 1] = mc.alpha;
        mcoef[4 * qi + 2] = mc.beta;
        mcoef[4 * qi + 3] = mc.gamma;
    }
}

// The int8 and float8 kernels take MASKED as a template parameter; their MASKED forms get the bitmap
// beside the arguments, and the unmasked forms keep the kernel arguments they had.
struct FilterArgsMasked {
    FilterArgs a;
    const uint32_t *mask;  // [ceil(r_end / 32)], over the local rows (BatchPlan::mask)
};
__device__ __forceinline__ const FilterArgs &filter_args(const FilterArgs &a) { return a; }
__device__ __forceinline__ const FilterArgs &filter_args(const FilterArgsMasked &m) { return m.a; }

// 256x256x64 tile, 512 threads = 8 waves in two groups (G0 = waves 0-3 own
// query rows 0-127, G1 = waves 4-7 rows 128-255; wave w and w+4 share a SIMD).
// Each wave owns 128 queries x 64 index rows as 4 quadrants of 64x32.  The
// (row tile, K-tile) steps of the block's chunk are one flattened sequence, so
// the next row tile's first K-tile streams in under the current tile's last
// MFMAs.  A K-tile is 4 phases; each phase is an M segment (ds_read the
// quadrant's fragments, issue this wave's LDS-DMA share of the next step,
// lgkmcnt(0)) and a C segment (16 MFMAs), each closed by a block barrier; G1
// runs one segment behind G0 so one wave per SIMD is in MFMAs while its partner
// reads LDS.  MFMA roles: A operand = index rows, B operand = queries, so a
// lane's accumulator holds 4 consecutive ROWS of one query: the epilogue tests
// one per-lane threshold against 16 values at a time.
// The body is filter_gemm_body.inc, included in the cosine kernel and in its METRIC form: one copy
// of the text, and the cosine kernel keeps the instructions it had.
template <typename T>
__global__ __launch_bounds__(512, 1) void filter_gemm_kernel(FilterArgs a) {
    constexpr bool METRIC = false, MASKED = false;
    [[maybe_unused]] const FilterMetric fm{};
    [[maybe_unused]] const uint32_t *const mask = nullptr;
    RC_FILTER_NOT_PAGED
#include "filter_gemm_body.inc"
}
template <typename T>
__global__ __launch_bounds__(512, 1) void filter_gemm_metric_kernel(FilterArgs a, FilterMetric fm) {
    constexpr bool METRIC = true, MASKED = false;
    [[maybe_unused]] const uint32_t *const mask = nullptr;
    RC_FILTER_NOT_PAGED
#include "filter_gemm_body.inc"
}
// the MASKED form of both (new kernels, so a template parameter costs no existing symbol; cosine: fm unused)
template <typename T, bool METRIC>
__global__ __launch_bounds__(512, 1) void filter_gemm_masked_kernel(FilterArgs a, FilterMetric fm, const uint32_t *mask) {
    constexpr bool MASKED = true;
    RC_FILTER_NOT_PAGED
#include "filter_gemm_body.inc"
}

// Query-stationary filter GEMM (ld = 64·NKT <= 512).  The filter GEMM above
// streams BOTH operands through LDS (256 queries x 256 rows per 64 KB K-step:
// 128 flop/B), which the L2->LDS fill rate caps near 45 % of MFMA peak.  Here a
// block's 256 queries live in REGISTERS for the whole launch and only index rows
// stream: one wave per SIMD (4 waves, up to 512 VGPRs each), wave w holds
// queries [64w, 64w+64) of the block's query group as 4 x 2·NKT B-fragments
// (256 VGPRs at ld 512) plus a 64 x 128 f32 accumulator (128 VGPRs).  Rows come
// in 128-row tiles, one 16 KB K-step (128 rows x 64) per stage of an 8-deep LDS
// ring (7 steps ≈ 112 KB in flight: enough to hide the HBM latency of a row
// tile's first touch): 2·256·128·64 flop per 16 KB = 256 flop/B, half the fill
// bytes of filter_gemm_kernel.  DMA through a per-step buffer descriptor (uniform
// base, 32-bit lane offsets) keeps addresses out of the VGPR budget.
// MFMA roles as above (A = index rows, B = queries): lane (li, g) of acc[rf][qt]
// holds rows 16·rf + 4g + j of query 16·qt + li.  Same thresholds, candidate
// appends and exactness argument as filter_gemm_kernel.
// Each wave holds 32 queries (2 x 16, QS_QT) for 128-row tiles: 8 waves, 2 per SIMD,
// every row-fragment read feeds two MFMAs and the SIMD partner wave's MFMAs cover
// its latency.  (A 4-wave form with 64 queries per wave pinned in AGPRs and
// inline-asm MFMAs was measured against it in round 2 — within 1 %, behind after
// the 2-GB sub-launches — and removed.)
// (QS_QT, QS_RT, QS_NS: filter_mfma.h)

// ABL (A/B diagnostics, diagnostic builds only; 0 in production): bit0 no DMA in the
// loop, bit1 no MFMA, bit2 no fragment reads (MFMAs on the query registers), bit3 no
// epilogue.
// The body is filter_qs_body.inc (as filter_gemm_body.inc); the METRIC form's epilogue loads the
// tile's norms itself.
template <typename T, int NKT, int ABL = 0>  // 256 queries per block
__global__ __launch_bounds__(512, 1) void filter_qs_kernel(FilterArgs a) {
    constexpr bool METRIC = false, MASKED = false;
    [[maybe_unused]] const FilterMetric fm{};
    [[maybe_unused]] const uint32_t *const mask = nullptr;
    RC_FILTER_NOT_PAGED
#include "filter_qs_body.inc"
}
template <typename T, int NKT>
__global__ __launch_bounds__(512, 1) void filter_qs_metric_kernel(FilterArgs a, FilterMetric fm) {
    constexpr bool METRIC = true, MASKED = false;
    constexpr int ABL = 0;
    [[maybe_unused]] const uint32_t *const mask = nullptr;
    RC_FILTER_NOT_PAGED
#include "filter_qs_body.inc"
}
// the MASKED form of both (as filter_gemm_masked_kernel)
template <typename T, int NKT, bool METRIC>
__global__ __launch_bounds__(512, 1) void filter_qs_masked_kernel(FilterArgs a, FilterMetric fm, const uint32_t *mask) {
    constexpr bool MASKED = true;
    constexpr int ABL = 0;
    RC_FILTER_NOT_PAGED
#include "filter_qs_body.inc"
}

// ------------------------------------------------ int8 filter (optional) --
// With the index's int8 filter copy (rc_index_set_filter(RC_FILTER_I8)) the filter GEMM
// runs on v_mfma_i32_16x16x64_i8 — twice the f16/bf16 MFMA rate, half the row bytes —
// and the candidates are still rescored exactly on the stored rows (rescore_kernel).
// A stored row x̂ is kept as x̃ = sx·x8 (x8 = rne(x̂/sx) in [-127, 127], sx = max|x̂|/127)
// with ex >= ||x̂ - x̃||₂; a normalised query qn as q̃ = sq·q8 with eq >= ||qn - q̃||₂.
// The integer dot D = q8·x8 is exact (|D| <= ld·127² < 2^24: exact in f32 too), and
//   |sq·sx·D - qn·x̂| <= ||qn||·ex + eq·||x̃|| <= ex·(1.0001 + eq) + 1.01·eq
// (||qn|| <= 1.0001, ||x̃|| <= ||x̂|| + ex, ||x̂|| <= 1.01).  A row is kept iff
//   sq·(sx·D) + ex·aq >= thr[q],   aq = 1.0001 + eq,   thr = kth - eps,
//   eps = 1.01·eq + 6.5e-5 (the f32 bound of the exact scores, as above) + 1e-6 (the
// f32 rounding of the left side), so the filter never drops a row of the final top-k.
// For unit rows in 512-d, ex and eq are ≈ 0.004-0.008: the candidate lists are a few
// times longer than with the f16 filter, so the stages grow more slowly
// (batch_stage_ratio's inflation).
//
// Queries: as prepare_queries_kernel (same qn arithmetic), plus q8 / sq / aq.
__global__ __launch_bounds__(64) void prepare_queries_i8_kernel(const float *__restrict__ q, int nq, int dim, int64_t ld,
                                                               float *__restrict__ qn, int8_t *__restrict__ q8,
                                                               float *__restrict__ sq, float *__restrict__ aq,
                                                               float *__restrict__ eps, float *__restrict__ thr) {
    const int lane = threadIdx.x;
    const int qi = blockIdx.x;
    const bool valid = qi < nq;
    const float *src = q + (int64_t)(valid ? qi : 0) * dim;
    const float inv = wave_inv_norm(src, dim, lane, valid);
    float mx = 0.f;
    for (int c = lane; c < ld; c += 64) {
        const float v = RC_UNIT_ELEM(src, c, dim, inv, valid);
        mx = fmaxf(mx, fabsf(v));
        if (valid) qn[(int64_t)qi * ld + c] = v;
    }
    mx = wave_max(mx);
    const float s = i8_scale(mx), is = i8_inv_scale(mx);  // quantised as the rows are (quantize_rows_kernel)
    float err = 0.f;
    for (int c = lane; c < ld; c += 64) {
        const float v = RC_UNIT_ELEM(src, c, dim, inv, valid);  // the value stored in qn above
        const float r = i8_round(v, is);
        q8[(int64_t)qi * ld + c] = (int8_t)r;
        const float d = v - s * r;
        err = fmaf(d, d, err);
    }
    err = wave_sum(err);
    if (lane == 0) {
        const float eq = i8_resid_bound(err);
        sq[qi] = s;
        aq[qi] = 1.0001f + eq;
        eps[qi] = 1.01f * eq + 6.6e-5f;
        thr[qi] = valid ? -INFINITY : INFINITY;
    }
}

// Query-stationary like filter_qs_kernel (same LDS ring, buffer-descriptor DMA, 128-row
// tiles, 8 waves x 32 queries), with the MFMA roles swapped: A = queries (registers),
// B = index rows (LDS), so lane (li, g) of acc[rf][qt] holds queries 16·qt + 4g + j of
// row 16·rf + li — one row per (lane, rf): its sx / ex are 8 values per lane per tile
// (i8_slot layout), loaded with the previous tile's epilogue.  A K-step is 128 bytes
// = 128 int8 elements, NKT = row bytes / 128 steps per tile.  Every ring step is
// issued (a step past the block's range reads nothing: zero-size buffer descriptor), so
// each wait counts a fixed number of younger loads: the DMA of the younger steps, plus
// this tile's 4 scale loads while they are younger than the awaited step.
// RT = rows per tile: 128, or 64 at ld 768 (NKT 6), where the 96 query-fragment registers
// leave room for only half the accumulators.
constexpr int I8_SL = 24;  // candidate rows staged in LDS per query per block (filter_i8_kernel)

// LDS atomic add / store as inline asm: written in C++, hipcc cannot tell these words from the
// LDS-DMA ring in the same __shared__ array and waits vmcnt(0) (the whole ring) before each one.
// The add's own lgkmcnt(0) is inside the statement, so its result is ready when it ends; the
// stores are retired by an explicit lgkmcnt(0) ahead of the block barrier before the flush.
__device__ __forceinline__ uint32_t lds_add_rtn_u32(uint32_t *p, uint32_t v) {
    uint32_t r;
    asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"((uint32_t)(uintptr_t)p), "v"(v) : "memory");
    return r;
}
__device__ __forceinline__ void lds_write_u32(uint32_t *p, uint32_t v) {
    asm volatile("ds_write_b32 %0, %1" ::"v"((uint32_t)(uintptr_t)p), "v"(v) : "memory");
}

// AUX: cache-policy bits of the row DMA (0; 2 = nontemporal: diagnostic builds' A/B)
// MASKED (the MASKED epilogues' comment above): here a lane holds ONE row per accumulator, row
// 16·rf + li of the tile, so its eligibility is one bit per rf (em).  The accumulators are integers:
// an ineligible row's become INT_MIN ahead of the gate's maximum, and since a huge negative value
// still passes v >= thr while thr is -inf, the append tests the row's bit as well.
template <int NKT, int RT, int AUX = 0, bool MASKED = false>
__global__ __launch_bounds__(512, 1) void filter_i8_kernel(std::conditional_t<MASKED, FilterArgsMasked, FilterArgs> am) {
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    const FilterArgs &a = filter_args(am);
    [[maybe_unused]] const uint32_t *mask = nullptr;
    if constexpr (MASKED) mask = am.mask;
    constexpr int QT = QS_QT, WAVES = 16 / QS_QT, RF = RT / 16, RH = RF / 4;
    constexpr int STEP_BYTES = RT * 128;
    constexpr int SPS = 2, SXL = 2 * RH;
    constexpr int PPW = 2 * RF / WAVES;
    static_assert((RT == 128 || RT == 64) && NKT % SPS == 0 && (QS_NS - 2 * SPS) * PPW + SXL < 64, "layout");
    // behind the ring (one __shared__ array): per query of the block a counter and I8_SL staged
    // candidate rows, appended with LDS atomics (lgkmcnt only) and flushed to the global lists
    // once at the block's end — a returning global atomic per append would wait for every
    // older vector-memory op, i.e. drain the DMA ring (vmcnt(0)) in the middle of the K loop
    __shared__ __attribute__((aligned(16))) uint8_t smem[QS_NS * STEP_BYTES + SB_TILE * 4 * (1 + I8_SL) + SB_TILE * 12];
    uint32_t *lcnt = reinterpret_cast<uint32_t *>(smem + QS_NS * STEP_BYTES);
    uint32_t *lbuf = lcnt + SB_TILE;
    // the block's per-query thr, sq, aq: read by each epilogue instead of held in 24 VGPRs, which
    // the K loop needs (in registers the kernel spilled; from LDS it is 0.7 % faster)
    float *lq = reinterpret_cast<float *>(lbuf + SB_TILE * I8_SL);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;

    const FilterBlock fb(a, RT);
    const int qb = fb.qb;
    const int64_t rt0 = fb.rt0, rt1 = fb.rt1;
    if (rt0 >= rt1) return;  // block-uniform
    const int64_t ldb = a.ld;  // bytes per row
    const int ntiles = (int)(rt1 - rt0);
    const int nsteps = ntiles * NKT;
    const int64_t row0 = a.r_begin + rt0 * RT;  // a multiple of RT (host check)
    const uint8_t *Rg = (const uint8_t *)a.rows + row0 * ldb;
    if (tid < SB_TILE) {  // visible to every wave after the K loop's first barrier
        const int q = qb * SB_TILE + tid;
        lcnt[tid] = 0u;
        lq[tid] = a.thr[q];
        lq[SB_TILE + tid] = a.sq[q];
        lq[2 * SB_TILE + tid] = a.aq[q];
    }

    i32x4_t qf[QT][2 * NKT];  // bytes [64 kk + 16 g, +16) of query q0 + 16 qt + li
    const int q0 = qb * SB_TILE + wave * 16 * QT;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int kk = 0; kk < 2 * NKT; ++kk)
            qf[qt][kk] = *reinterpret_cast<const i32x4_t *>((const uint8_t *)a.qh + (int64_t)(q0 + qt * 16 + li) * ldb +
                                                            kk * 64 + g * 16);
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int kk = 0; kk < 2 * NKT; ++kk) asm volatile("" ::"v"(qf[qt][kk]));
    // an epilogue's per-query operands: 3·QT LDS reads (inline asm: as C++, hipcc would wait for
    // the whole DMA ring first), retired together
    auto epi_params = [&](float (&thr)[QT][4], float (&sq)[QT][4], float (&aq)[QT][4]) __attribute__((always_inline)) {
        f32x4_t v[3][QT];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
                asm volatile("ds_read_b128 %0, %1"
                             : "=v"(v[c][qt])
                             : "v"((uint32_t)(uintptr_t)(lq + c * SB_TILE + wave * 16 * QT + qt * 16 + 4 * g)));
        static_assert(QT == 2, "the wait below ties 3 x 2 values");
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(v[0][0]), "+v"(v[0][1]), "+v"(v[1][0]), "+v"(v[1][1]), "+v"(v[2][0]), "+v"(v[2][1]));
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                thr[qt][j] = v[0][qt][j];
                sq[qt][j] = v[1][qt][j];
                aq[qt][j] = v[2][qt][j];
            }
    };

    uint32_t loff[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int r = (wave + WAVES * i) * 8 + (lane >> 3);
        loff[i] = (uint32_t)(r * (int)ldb + (((lane & 7) ^ ((r >> 1) & 7)) << 4));
    }
    auto issue = [&](int t) {
        const bool ok = t < nsteps;
        const int tile = t / NKT;
        const int ks = t - tile * NKT;
        uint8_t *base = smem + (t % QS_NS) * STEP_BYTES;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(ok ? Rg + (int64_t)tile * RT * ldb + ks * 128 : Rg), (short)0, ok ? 0x7fffffff : 0, 0x00020000);
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            lds_void *dst = (lds_void *)(base + (wave + WAVES * i) * 1024);
            const uint32_t off = loff[i];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst, 16, off, 0, 0, AUX);
        }
    };
    f32x4_t sxv[RH], exv[RH];  // rows 16 rf + li of the tile, rf = 4 h + e → sxv[h][e]
    auto load_scales = [&](int tile) {
        const int64_t tb = row0 + (int64_t)tile * RT;  // i8_slot(tb + 16 rf + li) = p + rf
        const int64_t p = (tb & ~int64_t(127)) + li * 8 + ((tb & 127) >> 4);
        asm volatile("" ::: "memory");
#pragma unroll
        for (int h = 0; h < RH; ++h) sxv[h] = *reinterpret_cast<const f32x4_t *>(a.rsx + p + 4 * h);
#pragma unroll
        for (int h = 0; h < RH; ++h) exv[h] = *reinterpret_cast<const f32x4_t *>(a.rex + p + 4 * h);
        asm volatile("" ::: "memory");
    };
    for (int t = 0; t < QS_NS - SPS; ++t) issue(t);
    load_scales(0);

    i32x4_t acc[RF][QT];
    for (int tile = 0; tile < ntiles; ++tile) {
        [[maybe_unused]] uint32_t mw[RT / 32];  // MASKED: the tile's bitmap words, loaded under its K loop
        if constexpr (MASKED) load_mask_words(mask, row0 + (int64_t)tile * RT, a.r_end, mw);
#pragma unroll
        for (int rf = 0; rf < RF; ++rf)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) acc[rf][qt] = i32x4_t{0, 0, 0, 0};
#pragma unroll
        for (int kp = 0; kp < NKT / SPS; ++kp) {
            const int t = tile * NKT + SPS * kp;
            // steps t..t+SPS-1 must have landed; younger: NS - 2·SPS steps, and this tile's
            // scale loads while they were issued after step t + SPS - 1
            if (t + QS_NS - SPS - 1 < nsteps) {
                if (SPS * (kp + 2) <= QS_NS)
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((QS_NS - 2 * SPS) * PPW + SXL) : "memory");
                else
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((QS_NS - 2 * SPS) * PPW) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
#pragma unroll
            for (int j = QS_NS - SPS; j < QS_NS; ++j) issue(t + j);
            constexpr int NG = SPS * 2 * RH;
            // row-fragment group gi: 4 rows-of-16 x (k-step kl, half sh) — read into cur, then 4 x QT
            // MFMAs.  Rolling schedule: each fragment of group gi + 1 is read as soon as the MFMAs
            // of the same slot of group gi have issued, so a group's LDS latency runs under the
            // previous group's MFMAs instead of in front of its own (no extra registers: the new
            // fragment takes the slot just freed).
            auto frag_addr = [&](int gi) {
                const int kl = gi / (2 * RH), sh = (gi / RH) % 2, rh = gi % RH;
                return smem + ((t + kl) % QS_NS) * STEP_BYTES + li * 128 + (((sh * 4 + g) ^ ((li >> 1) & 7)) << 4) +
                       rh * 4 * 2048;
            };
            i32x4_t cur[4];
            {
                const uint8_t *Sr = frag_addr(0);
#pragma unroll
                for (int i = 0; i < 4; ++i) cur[i] = *reinterpret_cast<const i32x4_t *>(Sr + i * 2048);
            }
            __builtin_amdgcn_sched_barrier(0);  // group 0's reads go out together, ahead of the pattern
#pragma unroll
            for (int gi = 0; gi < NG; ++gi) {
                const int kl = gi / (2 * RH), sh = (gi / RH) % 2, rh = gi % RH;
                const int ks = SPS * kp + kl;
                const uint8_t *Sn = frag_addr(gi + 1 < NG ? gi + 1 : gi);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt)
                        acc[rh * 4 + i][qt] =
                            __builtin_amdgcn_mfma_i32_16x16x64_i8(qf[qt][ks * 2 + sh], cur[i], acc[rh * 4 + i][qt], 0, 0, 0);
                    if (gi + 1 < NG) cur[i] = *reinterpret_cast<const i32x4_t *>(Sn + i * 2048);
                    __builtin_amdgcn_sched_group_barrier(0x008, QT, 0);
                    if (gi + 1 < NG) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
            }
        }
        // ---- epilogue: keep (q, row) iff sq·(sx·D) + ex·aq >= thr[q]
        [[maybe_unused]] uint32_t em = 0u;  // MASKED: bit rf = row 16 rf + li of the tile is eligible
        if constexpr (MASKED) {
            uint32_t any = 0u;
#pragma unroll
            for (int i = 0; i < RT / 32; ++i) any |= mw[i];
            if (any == 0u) {  // no eligible row in the tile: no epilogue (wave-uniform)
                load_scales(min(tile + 1, ntiles - 1));  // as at the tile's end: the same wait counts on every path
                continue;
            }
#pragma unroll
            for (int rf = 0; rf < RF; ++rf) {
                const bool el = ((mw[rf >> 1] >> ((rf & 1) * 16 + li)) & 1u) != 0u;
                em |= (uint32_t)el << rf;
#pragma unroll
                for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[rf][qt][j] = el ? acc[rf][qt][j] : INT_MIN;
            }
        }
        float sx[RF], ex[RF];
#pragma unroll
        for (int rf = 0; rf < RF; ++rf) {
            sx[rf] = sxv[rf >> 2][rf & 3];
            ex[rf] = exv[rf >> 2][rf & 3];
        }
        float exm = ex[0], sxmax = sx[0], sxmin = sx[0];
#pragma unroll
        for (int rf = 1; rf < RF; ++rf) {
            exm = fmaxf(exm, ex[rf]);
            sxmax = fmaxf(sxmax, sx[rf]);
            sxmin = fminf(sxmin, sx[rf]);
        }
        float thr[QT][4], sq[QT][4], aq[QT][4];
        epi_params(thr, sq, aq);
        // the gate: for every rf, sx[rf]·D[rf] <= sxb·Dmax with Dmax = max_rf D[rf] and sxb = sxmax
        // (Dmax >= 0) or sxmin (Dmax < 0); f32 products and the fma are monotonic, so the gate
        // passes whenever one of the lane's 8 per-element conditions below holds (the appends are
        // decided by those alone): an integer max per accumulator instead of cvt + mul + max
        bool hit = false, hq[QT][4];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int dm = acc[0][qt][j];
#pragma unroll
                for (int rf = 1; rf < RF; ++rf) dm = max(dm, acc[rf][qt][j]);
                const float m = (dm >= 0 ? sxmax : sxmin) * (float)dm;
                hq[qt][j] = fmaf(exm, aq[qt][j], sq[qt][j] * m) >= thr[qt][j];
                hit |= hq[qt][j];
            }
        if constexpr (MASKED) hit = hit && em != 0u;
        if (__ballot(hit) != 0 && hit) {
            const int64_t rbase = row0 + (int64_t)tile * RT + li;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // only the (qt, j) whose gate passed walk their 8 rows (the looser int8 bound
                    // sends about a quarter of the wave-tiles here)
                    if (!hq[qt][j]) continue;
                    const int q = q0 + qt * 16 + 4 * g + j;
#pragma unroll
                    for (int rf = 0; rf < RF; ++rf) {
                        const int64_t row = rbase + rf * 16;
                        const float v = fmaf(ex[rf], aq[qt][j], sq[qt][j] * (sx[rf] * (float)acc[rf][qt][j]));
                        if (v >= thr[qt][j] && (!MASKED || ((em >> rf) & 1u) != 0u) && row < a.r_end) {
                            const int ql = q - qb * SB_TILE;
                            const uint32_t p = lds_add_rtn_u32(&lcnt[ql], 1u);
                            if (p < (uint32_t)I8_SL) {
                                lds_write_u32(&lbuf[ql * I8_SL + p], (uint32_t)row);
                            } else {  // this block's slots of q are full: straight to the global list
                                append_candidate(a, q, row);
                            }
                        }
                    }
                }
        }
        load_scales(min(tile + 1, ntiles - 1));  // unconditional: the same wait counts on every path
    }
    // flush the staged candidates: one global atomic per query that has any.  The asm stores are
    // invisible to the compiler's wait-count tracking, so retire them explicitly before the barrier.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid < SB_TILE) {
        const uint32_t n = min(lcnt[tid], (uint32_t)I8_SL);
        if (n) {
            const int q = qb * SB_TILE + tid;
            const uint32_t base = atomicAdd(&a.cnt[q], n);
            for (uint32_t i = 0; i < n; ++i)
                if (base + i < (uint32_t)a.cap) a.cand[(int64_t)q * a.cap + base + i] = lbuf[tid * I8_SL + i];
        }
    }
}

// ------------------------------------------- float8 filter (RC_FILTER_F8) --
// A float8 index's own filter GEMM (rc_index_set_filter(RC_FILTER_F8)): it reads the stored e4m3
// bytes, no copy.  The instruction is the block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 with both
// operands e4m3 (twice the f16 MFMA rate at K = 128 per instruction); its E8M0 scale operands
// carry every power of two, exactly: 127 is 2⁰, the stored rows' 2⁻⁸ (F8_UNSCALE) is 119.
//
// Query in TERMS e4m3 terms.  One term (the storage rule applied to qn) leaves ||qn - q_hi|| ≈
// 0.026 for a unit query, a hundred times the f16 filter's rounding.  With two,
//   q_hi = e4m3(qn·2⁸)·2⁻⁸            (scale byte 119, the rows' rule: Elem<f8_t>::cast)
//   q_lo = e4m3((qn - q_hi)·2¹²)·2⁻¹²  (scale byte 115; |qn_c - q_hi,c| <= 2⁻⁴, so |·2¹²| <= 256 < 448)
// the residual ||qn - q_hi - q_lo|| is ≈ 6e-4, the f16 filter's order, and the stage ratio needs no
// inflation.  Both terms accumulate into the same accumulators: s' = (q_hi + q_lo)·x̂.
//
// Bound.  |s' - s| <= ||qn - q_hi - q_lo||·||x̂||max + c_acc, with ||x̂||max = 1.07 (a stored
// float8 row's norm is within 2⁻⁴ relative of 1) and c_acc = 6.5e-5 (the f32 chain of the exact
// score, as in the header) + c_mfma.  ASSUMPTION: the order and rounding of the MFMA's internal
// sums are not documented; c_mfma bounds them as a truncation (relative 2⁻²³) at every one of the
// ld products' additions and the TERMS·ld/128 accumulator additions of a score, on partial sums
// whose magnitude stays below ||q̃||·||x̂|| <= 1.07: c_mfma = (ld + TERMS·ld/128)·2⁻²³·1.07
// (1.0e-4 at ld 768).  rc_index_filter_scores exposes s' so that tests measure the real error
// against it.  eps[q] = 1.07·(residual norm, rounded up as i8_resid_bound) + c_acc, rounded up.
constexpr int F8_SCALE_ROWS = 119;  // E8M0 of F8_UNSCALE = 2⁻⁸: stored rows and q_hi
constexpr int F8_SCALE_QLO = 115;   // E8M0 of 2⁻¹²: q_lo
constexpr float F8_QLO_SCALE = 4096.0f, F8_QLO_UNSCALE = 1.0f / 4096.0f;
constexpr float F8_ROW_NORM_MAX = 1.07f;
__host__ __device__ constexpr float f8_filter_c_acc(int64_t ld, int terms) {
    return 6.5e-5f + (float)(ld + terms * (ld / 128)) * (1.0f / 8388608.0f) * F8_ROW_NORM_MAX;
}

// Queries: qn exactly as prepare_queries_kernel forms it (the rescored bits stay the scan's), the
// two e4m3 planes qh[0] = q_hi, qh[1] = q_lo ([nq_pad][ld] bytes each; TERMS = 1: q_lo is not
// written and the residual is qn - q_hi), eps and thr.
template <int TERMS>
__global__ __launch_bounds__(64) void prepare_queries_f8_kernel(const float *__restrict__ q, int nq, int dim, int64_t ld,
                                                               int64_t plane, float *__restrict__ qn, f8_t *__restrict__ qh,
                                                               float *__restrict__ eps, float *__restrict__ thr) {
    const int lane = threadIdx.x;
    const int qi = blockIdx.x;
    const bool valid = qi < nq;
    const float *src = q + (int64_t)(valid ? qi : 0) * dim;
    const float inv = wave_inv_norm(src, dim, lane, valid);
    float err = 0.f;
    for (int c = lane; c < ld; c += 64) {
        const float v = RC_UNIT_ELEM(src, c, dim, inv, valid);
        const f8_t hi = Elem<f8_t>::cast(v);
        float d = v - Elem<f8_t>::load(&hi, 0);
        qh[(int64_t)qi * ld + c] = hi;
        if constexpr (TERMS == 2) {
            const uint8_t lo = (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(d * F8_QLO_SCALE, 0.f, 0, false) & 0xff);
            d -= __builtin_amdgcn_cvt_f32_fp8((int)lo, 0) * F8_QLO_UNSCALE;
            qh[plane + (int64_t)qi * ld + c] = f8_t{lo};
        }
        err = fmaf(d, d, err);
        if (valid) qn[(int64_t)qi * ld + c] = v;
    }
    err = wave_sum(err);
    if (lane == 0) {
        eps[qi] = (F8_ROW_NORM_MAX * i8_resid_bound(err) + f8_filter_c_acc(ld, TERMS)) * 1.0001f;
        thr[qi] = valid ? -INFINITY : INFINITY;
    }
}

struct FilterF8Args {
    FilterArgs a;         // rows: the stored e4m3 rows; qh: the q_hi plane; ld = bytes per row; nqb: blocks of 128·QT queries
    const uint8_t *qlo;   // the q_lo plane (TERMS 2)
    float *dump;          // DUMP: s' of queries [0, dump_nq) x rows [r_begin, r_end), [dump_nq][r_end - r_begin]
    int dump_nq;
};
struct FilterF8ArgsMasked {  // the MASKED form's (as FilterArgsMasked)
    FilterF8Args f;
    const uint32_t *mask;
};
__device__ __forceinline__ const FilterF8Args &filter_args(const FilterF8Args &f) { return f; }
__device__ __forceinline__ const FilterF8Args &filter_args(const FilterF8ArgsMasked &m) { return m.f; }

// Query-stationary, as filter_qs_kernel / filter_i8_kernel: same FilterBlock mapping, 8 waves, the
// same LDS ring of RT rows x 128 B per step filled by buffer-descriptor DMA, every ring step issued
// (past the block's range through a zero-size descriptor) so that each wait counts a fixed number
// of younger loads.  One ring step is one MFMA K: 128 bytes = 128 e4m3 elements.  A wave holds
// 16·QT queries as TERMS x NKT fragments of 8 VGPRs per query tile (NKT = ld / 128).
// MFMA roles as filter_qs_kernel (A = index rows from LDS, B = queries in registers): lane
// (li, g) of acc[rf][qt] holds rows 16·rf + 4g + j of query 16·qt + li; one threshold per
// (lane, qt), the same two-level epilogue.
// Operand bytes: lane (li, g) supplies 32 bytes for row / query li.  Only consistency matters
// (the k indices a lane's bytes stand for are the same set for A and for B, whichever the
// hardware assigns them, and both scales are uniform): both sides give bytes [32g, 32g + 32) of
// the 128-byte K chunk in memory order — the query from global memory, the row fragment from LDS
// as the 16-B chunks 2g and 2g + 1 of row 16·rf + li.  LDS layout as the other two kernels: chunk c
// of row r at position c ^ ((r >> 1) & 7) of the row's 128 bytes.  Bank conflicts: a quarter-wave
// is 16 lanes of one g, rows li = 0..15; its 16-B reads sit at bank (li & 1)·32 + 4·((2g + h) ^
// (li >> 1)): the 8 values of li >> 1 give 8 distinct positions in each half of the 64 banks, so
// the 16 lanes cover all 64 banks once — no conflict, for either chunk h.
// Registers (256 per lane at 2 waves per SIMD): query fragments TERMS·NKT·8·QT, accumulators
// RT/16·QT·4, GF row-fragment slots of 8 (2 slots where the query fragments take 128, else 4).
//   ld 256: QT 2, RT 128:  64 + 64 + 32, 207 VGPRs in all
//   ld 512: QT 2, RT  64: 128 + 32 + 16, 221 (RT 128 needs 256 and spills 84 bytes)
//   ld 768: QT 1, RT  64:  96 + 16 + 32, 170 (QT 2 would hold 192 in query fragments alone: a block
//           is 128 queries there, and a row-fragment read feeds 2 MFMAs instead of 4)
// No instantiation uses scratch.  The ring is NS = 8 steps of 128 rows or 16 steps of 64: 128 KB.
// DUMP (rc_index_filter_scores): the epilogue stores s' instead of testing it; the fragment
// loads, the ring and the MFMAs are the product's.
typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef int i32x4v_t __attribute__((ext_vector_type(4)));

// acc + (stored-row fragment, scale 2⁻⁸) x (query fragment, E8M0 scale byte qscale), both e4m3.  The
// scale words hold the byte in all four bytes, so any op_sel reads it.
__device__ __forceinline__ f32x4_t mfma_f8_scaled(i32x8_t row, i32x8_t query, f32x4_t acc, int qscale) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(row, query, acc, 0, 0, 0, F8_SCALE_ROWS * 0x01010101, 0,
                                                            qscale * 0x01010101);
}

// MASKED (the MASKED epilogues' comment above): rows and accumulators as filter_qs_kernel's, so the
// same 4-bit fields.  No MASKED DUMP form.
template <int NKT, int RT, int TERMS, int QT, bool DUMP = false, bool MASKED = false>
__global__ __launch_bounds__(512, 1) void filter_f8_kernel(std::conditional_t<MASKED, FilterF8ArgsMasked, FilterF8Args> fam) {
    static_assert(!(DUMP && MASKED), "the DUMP form has no mask");
    const FilterF8Args &fa = filter_args(fam);
    [[maybe_unused]] const uint32_t *mask = nullptr;
    if constexpr (MASKED) mask = fam.mask;
    constexpr int WAVES = 8, QPB = WAVES * 16 * QT, RF = RT / 16, RH = RF / 4;
    constexpr int STEP_BYTES = RT * 128;
    constexpr int NS = QS_NS * 128 / RT;  // ring steps: 128 KB of rows either way
    constexpr int SPS = 2;
    constexpr int PPW = 2 * RF / WAVES;
    constexpr int GF = TERMS * NKT * QT * 8 >= 128 ? 2 : 4;  // row-fragment register slots (8 VGPRs each)
    static_assert((RT == 128 || RT == 64) && (TERMS == 1 || TERMS == 2) && NKT % SPS == 0 && (NS - 2 * SPS) * PPW < 64,
                  "layout; vmcnt is 6 bits");
    __shared__ __attribute__((aligned(16))) uint8_t smem[NS * STEP_BYTES];
    const FilterArgs &a = fa.a;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;

    const FilterBlock fb(a, RT);
    const int qb = fb.qb;
    const int64_t rt0 = fb.rt0, rt1 = fb.rt1;
    if (rt0 >= rt1) return;  // block-uniform
    const int64_t ldb = a.ld;  // bytes per row
    const int ntiles = (int)(rt1 - rt0);
    const int nsteps = ntiles * NKT;
    const int64_t row0 = a.r_begin + rt0 * RT;  // a multiple of RT (host check)
    const uint8_t *Rg = (const uint8_t *)a.rows + row0 * ldb;

    // this lane's query fragments for the whole K: bytes [128 ks + 32 g, + 32) of query q0 + 16 qt + li
    i32x8_t qf[TERMS][QT][NKT];
    const int q0 = qb * QPB + wave * 16 * QT;
#pragma unroll
    for (int tm = 0; tm < TERMS; ++tm)
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int ks = 0; ks < NKT; ++ks) {
                const uint8_t *src = (tm == 0 ? (const uint8_t *)a.qh : fa.qlo) + (int64_t)(q0 + qt * 16 + li) * ldb + ks * 128 + g * 32;
                qf[tm][qt][ks] = *reinterpret_cast<const i32x8_t *>(src);  // 32-B aligned: two 16-B loads into one tuple
            }
    float thr[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) thr[qt] = a.thr[q0 + qt * 16 + li];
    // consume the query loads here: the compiler's vmcnt waits for them sit before the K loop
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        asm volatile("" ::"v"(thr[qt]));
#pragma unroll
        for (int tm = 0; tm < TERMS; ++tm)
#pragma unroll
            for (int ks = 0; ks < NKT; ++ks) {
                // (in 16-byte halves: a 32-byte "v" operand is no operand of the host pass's target, and
                // in a template that drops the kernel's stub without a diagnostic)
                const i32x4v_t h0 = __builtin_shufflevector(qf[tm][qt][ks], qf[tm][qt][ks], 0, 1, 2, 3);
                const i32x4v_t h1 = __builtin_shufflevector(qf[tm][qt][ks], qf[tm][qt][ks], 4, 5, 6, 7);
                asm volatile("" ::"v"(h0), "v"(h1));
            }
    }

    uint32_t loff[PPW];  // byte offset of this lane's 16 B within the step's rows
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int r = (wave + WAVES * i) * 8 + (lane >> 3);
        loff[i] = (uint32_t)(r * (int)ldb + (((lane & 7) ^ ((r >> 1) & 7)) << 4));
    }
    auto issue = [&](int t) {
        const bool ok = t < nsteps;
        const int tile = t / NKT;
        const int ks = t - tile * NKT;
        uint8_t *base = smem + (t % NS) * STEP_BYTES;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(ok ? Rg + (int64_t)tile * RT * ldb + ks * 128 : Rg), (short)0, ok ? 0x7fffffff : 0, 0x00020000);
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            lds_void *dst = (lds_void *)(base + (wave + WAVES * i) * 1024);
            const uint32_t off = loff[i];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst, 16, off, 0, 0, 0);
        }
    };
    for (int t = 0; t < NS - SPS; ++t) issue(t);

    f32x4_t acc[RF][QT];
    for (int tile = 0; tile < ntiles; ++tile) {
        [[maybe_unused]] uint32_t mw[RT / 32];  // MASKED: the tile's bitmap words, loaded under its K loop
        if constexpr (MASKED) load_mask_words(mask, row0 + (int64_t)tile * RT, a.r_end, mw);
#pragma unroll
        for (int rf = 0; rf < RF; ++rf)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) acc[rf][qt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kp = 0; kp < NKT / SPS; ++kp) {
            const int t = tile * NKT + SPS * kp;
            // steps t..t+SPS-1 must have landed; the NS - 2·SPS younger steps (PPW DMAs each, always
            // issued) may be in flight.  What an epilogue issued (atomics, stores) only makes the
            // wait stricter.
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2 * SPS) * PPW) : "memory");
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();  // every wave's DMA of t..t+SPS-1 landed; slots of t-SPS..t-1 are free
            asm volatile("" ::: "memory");
#pragma unroll
            for (int j = NS - SPS; j < NS; ++j) issue(t + j);
            // The sync group's SPS·RF row fragments f = (k-step kl, row group rf), GF register slots,
            // rolling as filter_i8_kernel: fragment f + GF is read into the slot of fragment f as soon as
            // f's QT·TERMS MFMAs have issued, so its LDS latency runs under the MFMAs between.  Row
            // r = 16 rf + li: its swizzle (r >> 1) & 7 = (li >> 1) & 7 does not depend on rf.
            constexpr int NF = SPS * RF;
            const int sw = (li >> 1) & 7;
            auto read_frag = [&](int f) {
                const int kl = f / RF, rf = f % RF;
                const uint8_t *Sr = smem + ((t + kl) % NS) * STEP_BYTES + (16 * rf + li) * 128;
                const i32x4v_t lo = *reinterpret_cast<const i32x4v_t *>(Sr + (((2 * g) ^ sw) << 4));
                const i32x4v_t hi = *reinterpret_cast<const i32x4v_t *>(Sr + (((2 * g + 1) ^ sw) << 4));
                return (i32x8_t)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            };
            i32x8_t cur[GF];
#pragma unroll
            for (int f = 0; f < GF; ++f) cur[f] = read_frag(f);
            __builtin_amdgcn_sched_barrier(0);  // the first GF fragments' reads go out together, ahead of the pattern
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const int ks = SPS * kp + f / RF, rf = f % RF;
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    acc[rf][qt] = mfma_f8_scaled(cur[f % GF], qf[0][qt][ks], acc[rf][qt], F8_SCALE_ROWS);
                    if constexpr (TERMS == 2)
                        acc[rf][qt] = mfma_f8_scaled(cur[f % GF], qf[TERMS - 1][qt][ks], acc[rf][qt], F8_SCALE_QLO);
                }
                if (f + GF < NF) cur[f % GF] = read_frag(f + GF);
                __builtin_amdgcn_sched_group_barrier(0x008, QT * TERMS, 0);
                if (f + GF < NF) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            }
            // pin the accumulators here: the step issue's branches split the basic block, and the
            // compiler otherwise sinks this sync group's MFMAs into the next one's block, where all of
            // its row fragments stay live at once (128 registers; the kernel spilled)
#pragma unroll
            for (int rf = 0; rf < RF; ++rf)
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) asm volatile("" : "+v"(acc[rf][qt]));
        }
        // rows in 32 bits from here (a local row is below the capacity, < 2^32): the tile's first row
        // of this lane, and how many rows from it are inside the range
        const uint32_t rbase = (uint32_t)(row0 + (int64_t)tile * RT) + 4u * (uint32_t)g;
        const int64_t left64 = a.r_end - (row0 + (int64_t)tile * RT) - 4 * g;
        const int left = (int)(left64 < RT ? left64 : RT);  // row rbase + o is in range iff o < left
        if constexpr (DUMP) {  // rc_index_filter_scores: s' itself
            const int64_t n = a.r_end - a.r_begin;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                const int q = q0 + qt * 16 + li;
                float *dst = fa.dump + (int64_t)q * n + ((int64_t)rbase - a.r_begin);
#pragma unroll
                for (int rf = 0; rf < RF; ++rf)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (q < fa.dump_nq && rf * 16 + j < left) dst[rf * 16 + j] = acc[rf][qt][j];
            }
            continue;
        }
        // ---- epilogue of the tile: candidates s' >= thr[q]
        if constexpr (MASKED) {
            uint32_t any = 0u;
#pragma unroll
            for (int i = 0; i < RT / 32; ++i) any |= mw[i];
            if (any == 0u) continue;  // no eligible row in the tile: no epilogue (wave-uniform)
#pragma unroll
            for (int rf = 0; rf < RF; ++rf) {
                const uint32_t e = mw[rf >> 1] >> ((rf & 1) * 16 + 4 * g);  // rows 16 rf + 4 g + j: bit j
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) acc[rf][qt] = mask_ineligible4(acc[rf][qt], e);
            }
        }
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            const float th = thr[qt];
            float m = -INFINITY;
#pragma unroll
            for (int rf = 0; rf < RF; ++rf) {
                const f32x4_t v = acc[rf][qt];
                m = fmaxf(m, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
            }
            if (__ballot(m >= th) == 0) continue;  // wave-uniform: the common case
            if (m >= th) {
                const int q = q0 + qt * 16 + li;
#pragma unroll
                for (int rf = 0; rf < RF; ++rf)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (acc[rf][qt][j] >= th && rf * 16 + j < left) append_candidate(a, q, (int64_t)(rbase + (uint32_t)(rf * 16 + j)));
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the zero-size tail steps of the ring
}

// ------------------------------------------------------- exact rescoring --
// rescore_kernel and its metric form are in rescore.h; the metric kernels are instantiated in
// rescore_metric_{f16,bf16}.hip, not here.
extern template void launch_rescore_metric<f16_t>(const BatchPlan &, const BatchWs &, int, hipStream_t);
extern template void launch_rescore_metric<bf16_t>(const BatchPlan &, const BatchWs &, int, hipStream_t);
// ... and the page-table form of both (BatchPlan::pages) in rescore_paged_{f16,bf16}.hip
extern template void launch_rescore_paged<f16_t>(const BatchPlan &, const BatchWs &, int, hipStream_t);
extern template void launch_rescore_paged<bf16_t>(const BatchPlan &, const BatchWs &, int, hipStream_t);

// ------------------------------------------------------------------ host ---
template <typename T>
void launch_rescore(const BatchPlan &p, const BatchWs &ws, int final_pass, hipStream_t s) {
    if constexpr (sizeof(T) == 2) {  // the metric filter's dtypes: f16 / bf16
        if (p.pages != nullptr) return launch_rescore_paged<T>(p, ws, final_pass, s);  // candidates are positions
        if (p.metric != RC_METRIC_COSINE) return launch_rescore_metric<T>(p, ws, final_pass, s);
    }
    // (float8 rows: the even widths up to 768, what the float8 filter serves)
    const bool ok = with_nch<(sizeof(T) == 1 ? 6 : 16), T>(p.nch, [&](auto nch) {
        with_topk_cap(topk_cap(p.k), [&](auto cap) {
            auto launch = [&](auto masked) {
                hipLaunchKernelGGL((rescore_kernel<T, decltype(nch)::value, decltype(cap)::value, decltype(masked)::value>),
                                   dim3(p.nq), dim3(256), 0, s, (const T *)p.rows, p.ld, ws.qn, p.k, ws.cnt, ws.cand, ws.cap, ws.keys,
                                   ws.eps, ws.thr, ws.flags, ws.ovf, final_pass, p.row_base, p.row_stride, p.out_scores, p.out_rows,
                                   p.mask);
            };
            if (p.mask != nullptr) launch(std::true_type{});
            else launch(std::false_type{});
        });
    });
    if (!ok) throw Error(RC_ERR_UNSUPPORTED, "unsupported row width");
    RC_LAUNCH_CHECK();
}

int batch_stage_ratio(int k, int cap, int inflation) {
    const int g = cap / (5 * k / 2 * inflation + 1);
    return std::max(2, std::min(64, g));
}

// The stages: stage 1 takes the first cap rows as candidates (thr = -inf), each later
// stage filters the next g-times-larger row range against the running thresholds, then
// rescore_kernel merges its candidates.  filter(c0, c1, nchunk) enqueues one filter
// dispatch over rows [c0, c1) split into nchunk row chunks.
#if defined(RC_GEMM_ABLATION)
int g_diag_filter_split_log2 = 31;
int g_diag_filter_aux = 0;  // the int8 filter's row DMA cache policy (rc_diag_set_filter_aux)
#endif
template <typename T, typename F>
void run_stages(const BatchPlan &p, BatchWs &ws, hipStream_t s, KernelTimer *timer, int g, int64_t row_bytes, F &&filter) {
    const int nqb = (p.nq + SB_TILE - 1) / SB_TILE;
    const int nq_pad = nqb * SB_TILE;
    RC_HIP(hipMemsetAsync(ws.keys, 0xFF, (size_t)p.nq * p.k * sizeof(uint64_t), s));
    RC_HIP(hipMemsetAsync(ws.cnt, 0, (size_t)nq_pad * sizeof(uint32_t), s));
    RC_HIP(hipMemsetAsync(ws.flags, 0, (size_t)p.nq * sizeof(int), s));
    int64_t b0 = 0, b1 = std::min<int64_t>(p.n_rows, ws.cap);
    // With nq > 256 the nqb query blocks that read one row chunk run side by side on one
    // XCD so that its L2 serves the second to last reader; over a long chunk their
    // progress drifts apart by more than the L2 holds (memory-side reads 2.8x the rows
    // at 125M rows).  Sub-launches of <= 2 GB of rows realign them: reads fall to 1.05x
    // and the filter runs 3-5 % faster (profiles/r02/r02_ab_results.txt).
#if defined(RC_GEMM_ABLATION)
    const int split_log2 = g_diag_filter_split_log2;  // diagnostic builds: the sub-launch size A/B
#else
    constexpr int split_log2 = 31;
#endif
    const int64_t split = nqb > 1 ? std::max<int64_t>(SB_TILE, ((int64_t)1 << split_log2) / row_bytes / SB_TILE * SB_TILE)
                                  : (int64_t)0;
    while (b0 < p.n_rows) {
        for (int64_t c0 = b0; c0 < b1;) {
            const int64_t c1 = split > 0 ? std::min(b1, c0 + split) : b1;
            const int slot = timer ? timer->begin(s) : -1;  // per dispatch, as rocprofv3 counts them
            const int64_t rt_total = (c1 - c0 + SB_TILE - 1) / SB_TILE;
            int64_t nchunk = std::min<int64_t>(rt_total, std::max<int64_t>(1, (256 + nqb - 1) / nqb));
            nchunk = (nchunk + 7) / 8 * 8;
            filter(c0, c1, nchunk, nqb);
            RC_LAUNCH_CHECK();
            if (timer) timer->end(slot, s, 2.0 * (double)nq_pad * (double)(c1 - c0) * (double)p.ld);
            c0 = c1;
        }
        launch_rescore<T>(p, ws, b1 == p.n_rows ? 1 : 0, s);
        b0 = b1;
        b1 = std::min<int64_t>(p.n_rows, b1 * g);
    }
}

template <typename T>
void run_batched(const BatchPlan &p, BatchWs &ws, hipStream_t s, KernelTimer *timer) {
    const int nq_pad = (p.nq + SB_TILE - 1) / SB_TILE * SB_TILE;
    const bool metric = p.metric != RC_METRIC_COSINE;  // the METRIC forms of the same kernels (RC_FILTER_METRIC)
    if (metric)
        hipLaunchKernelGGL(prepare_queries_metric_kernel<T>, dim3(nq_pad), dim3(64), 0, s, p.queries, p.nq, p.dim, p.ld, p.metric,
                           ws.qn, (T *)ws.qh, ws.eps, ws.thr, ws.mcoef);
    else
        hipLaunchKernelGGL(prepare_queries_kernel<T>, dim3(nq_pad), dim3(64), 0, s, p.queries, p.nq, p.dim, p.ld, ws.qn,
                           (T *)ws.qh, ws.eps, ws.thr);
    RC_LAUNCH_CHECK();
    auto filter = [&](int64_t c0, int64_t c1, int64_t nchunk, int nqb) {
        const int64_t rt_total = (c1 - c0 + SB_TILE - 1) / SB_TILE;
        const int64_t tpc = (rt_total + nchunk - 1) / nchunk;
        FilterArgs fa{p.rows, ws.qh, p.ld, (int)(p.ld / 64), c0, c1, tpc, nqb, ws.thr, ws.cnt, ws.cand, ws.cap};
        const int nkt = (int)(p.ld / 64);
        if (p.pages != nullptr) return launch_filter_paged<T>(p, ws, fa, nchunk, nqb, s);  // the PAGED forms (search_mfma_paged.hip)
        if (p.mask_filter) {  // RC_SEARCH_MFMA_MASKED: the MASKED forms (cosine: fm is not read)
            const FilterMetric fm{p.norms, ws.mcoef};
            auto launch = [&](auto m) {
                constexpr bool M = decltype(m)::value;
                if (nkt == 2 || nkt == 4 || nkt == 8) {
                    fa.tiles_per_chunk = ((c1 - c0 + QS_RT - 1) / QS_RT + nchunk - 1) / nchunk;
                    const dim3 gr((unsigned)(nchunk * nqb)), bl(64 * 16 / QS_QT);
                    if (nkt == 8) hipLaunchKernelGGL((filter_qs_masked_kernel<T, 8, M>), gr, bl, 0, s, fa, fm, p.mask);
                    else if (nkt == 4) hipLaunchKernelGGL((filter_qs_masked_kernel<T, 4, M>), gr, bl, 0, s, fa, fm, p.mask);
                    else hipLaunchKernelGGL((filter_qs_masked_kernel<T, 2, M>), gr, bl, 0, s, fa, fm, p.mask);
                } else {
                    hipLaunchKernelGGL((filter_gemm_masked_kernel<T, M>), dim3((unsigned)(nchunk * nqb)), dim3(512), 0, s, fa, fm,
                                       p.mask);
                }
            };
            if (metric) launch(std::true_type{});
            else launch(std::false_type{});
            return;
        }
        if (metric) {
            const FilterMetric fm{p.norms, ws.mcoef};
            if (nkt == 2 || nkt == 4 || nkt == 8) {
                fa.tiles_per_chunk = ((c1 - c0 + QS_RT - 1) / QS_RT + nchunk - 1) / nchunk;
                const dim3 gr((unsigned)(nchunk * nqb)), bl(64 * 16 / QS_QT);
                if (nkt == 8) hipLaunchKernelGGL((filter_qs_metric_kernel<T, 8>), gr, bl, 0, s, fa, fm);
                else if (nkt == 4) hipLaunchKernelGGL((filter_qs_metric_kernel<T, 4>), gr, bl, 0, s, fa, fm);
                else hipLaunchKernelGGL((filter_qs_metric_kernel<T, 2>), gr, bl, 0, s, fa, fm);
            } else {
                hipLaunchKernelGGL(filter_gemm_metric_kernel<T>, dim3((unsigned)(nchunk * nqb)), dim3(512), 0, s, fa, fm);
            }
            return;
        }
        if (nkt == 2 || nkt == 4 || nkt == 8) {
            fa.tiles_per_chunk = ((c1 - c0 + QS_RT - 1) / QS_RT + nchunk - 1) / nchunk;
            const dim3 gr((unsigned)(nchunk * nqb)), bl(64 * 16 / QS_QT);
            if (nkt == 8) hipLaunchKernelGGL((filter_qs_kernel<T, 8>), gr, bl, 0, s, fa);
            else if (nkt == 4) hipLaunchKernelGGL((filter_qs_kernel<T, 4>), gr, bl, 0, s, fa);
            else hipLaunchKernelGGL((filter_qs_kernel<T, 2>), gr, bl, 0, s, fa);
        } else {
            hipLaunchKernelGGL(filter_gemm_kernel<T>, dim3((unsigned)(nchunk * nqb)), dim3(512), 0, s, fa);
        }
    };
    run_stages<T>(p, ws, s, timer, batch_stage_ratio(p.k, ws.cap), p.ld * (int64_t)sizeof(T), filter);
}

// Candidates per stage grow by exp(z·eps/σ) over the f16 filter's (≈ 3x for random unit
// rows in 512-d at top-100 of 125M); the stage ratio assumes 3x.
constexpr int I8_STAGE_INFLATION = 3;

template <typename T>
void run_batched_i8(const BatchPlan &p, BatchWs &ws, hipStream_t s, KernelTimer *timer) {
    const int nq_pad = (p.nq + SB_TILE - 1) / SB_TILE * SB_TILE;
    hipLaunchKernelGGL(prepare_queries_i8_kernel, dim3(nq_pad), dim3(64), 0, s, p.queries, p.nq, p.dim, p.ld, ws.qn,
                       (int8_t *)ws.qh, ws.sq, ws.aq, ws.eps, ws.thr);
    RC_LAUNCH_CHECK();
    const int nkt = (int)(p.ld / 128);
    auto filter = [&](int64_t c0, int64_t c1, int64_t nchunk, int nqb) {
        const int rt = nkt == 6 ? 64 : 128;
        RC_REQUIRE(c0 % rt == 0, RC_ERR_INVALID, "internal: int8 filter range not tile-aligned");
        const int64_t tpc = ((c1 - c0 + rt - 1) / rt + nchunk - 1) / nchunk;
        FilterArgs fa{p.rows8, ws.qh, p.ld, nkt, c0, c1, tpc, nqb, ws.thr, ws.cnt, ws.cand, ws.cap};
        fa.rsx = p.rsx;
        fa.rex = p.rex;
        fa.sq = ws.sq;
        fa.aq = ws.aq;
        const dim3 gr((unsigned)(nchunk * nqb)), bl(64 * 16 / QS_QT);
        if (p.mask_filter) {  // RC_SEARCH_MFMA_MASKED
            const FilterArgsMasked fm{fa, p.mask};
            if (nkt == 4) hipLaunchKernelGGL((filter_i8_kernel<4, 128, 0, true>), gr, bl, 0, s, fm);
            else if (nkt == 6) hipLaunchKernelGGL((filter_i8_kernel<6, 64, 0, true>), gr, bl, 0, s, fm);
            else hipLaunchKernelGGL((filter_i8_kernel<2, 128, 0, true>), gr, bl, 0, s, fm);
            return;
        }
#if defined(RC_GEMM_ABLATION)
        if (nkt == 4 && g_diag_filter_aux == 2) {
            hipLaunchKernelGGL((filter_i8_kernel<4, 128, 2>), gr, bl, 0, s, fa);
            return;
        }
#endif
        if (nkt == 4) hipLaunchKernelGGL((filter_i8_kernel<4, 128>), gr, bl, 0, s, fa);
        else if (nkt == 6) hipLaunchKernelGGL((filter_i8_kernel<6, 64>), gr, bl, 0, s, fa);
        else hipLaunchKernelGGL((filter_i8_kernel<2, 128>), gr, bl, 0, s, fa);
    };
    run_stages<T>(p, ws, s, timer, batch_stage_ratio(p.k, ws.cap, I8_STAGE_INFLATION), p.ld, filter);
}

// The float8 filter (filter_f8_kernel): two e4m3 query terms, no stage inflation.  ld 768 runs
// QT = 1 (blocks of 128 queries): its 192 query-fragment registers at QT = 2 leave no room.
constexpr int F8_TERMS = 2;

// launch filter_f8_kernel<.., DUMP> over rows [c0, c1) in nchunk row chunks for nq_pad query slots
template <bool DUMP>
void launch_filter_f8(const BatchPlan &p, const BatchWs &ws, int nq_pad, int64_t c0, int64_t c1, int64_t nchunk, float *dump,
                      hipStream_t s) {
    const int nkt = (int)(p.ld / 128);
    const int rt = nkt >= 4 ? 64 : 128, qt = nkt == 6 ? 1 : QS_QT;
    const int nqb = nq_pad / (128 * qt);
    RC_REQUIRE(c0 % rt == 0, RC_ERR_INVALID, "internal: float8 filter range not tile-aligned");
    const int64_t tpc = ((c1 - c0 + rt - 1) / rt + nchunk - 1) / nchunk;
    FilterF8Args fa{FilterArgs{p.rows, ws.qh, p.ld, nkt, c0, c1, tpc, nqb, ws.thr, ws.cnt, ws.cand, ws.cap},
                    (const uint8_t *)ws.qh + (int64_t)nq_pad * p.ld, dump, p.nq};
    const dim3 gr((unsigned)(nchunk * nqb)), bl(512);
    if constexpr (!DUMP) {
        if (p.mask_filter) {  // RC_SEARCH_MFMA_MASKED
            const FilterF8ArgsMasked fm{fa, p.mask};
            if (nkt == 4) hipLaunchKernelGGL((filter_f8_kernel<4, 64, F8_TERMS, QS_QT, false, true>), gr, bl, 0, s, fm);
            else if (nkt == 6) hipLaunchKernelGGL((filter_f8_kernel<6, 64, F8_TERMS, 1, false, true>), gr, bl, 0, s, fm);
            else hipLaunchKernelGGL((filter_f8_kernel<2, 128, F8_TERMS, QS_QT, false, true>), gr, bl, 0, s, fm);
            return;
        }
    }
    if (nkt == 4) hipLaunchKernelGGL((filter_f8_kernel<4, 64, F8_TERMS, QS_QT, DUMP>), gr, bl, 0, s, fa);
    else if (nkt == 6) hipLaunchKernelGGL((filter_f8_kernel<6, 64, F8_TERMS, 1, DUMP>), gr, bl, 0, s, fa);
    else hipLaunchKernelGGL((filter_f8_kernel<2, 128, F8_TERMS, QS_QT, DUMP>), gr, bl, 0, s, fa);
}

void prepare_queries_f8(const BatchPlan &p, const BatchWs &ws, int nq_pad, hipStream_t s) {
    hipLaunchKernelGGL(prepare_queries_f8_kernel<F8_TERMS>, dim3(nq_pad), dim3(64), 0, s, p.queries, p.nq, p.dim, p.ld,
                       (int64_t)nq_pad * p.ld, ws.qn, (f8_t *)ws.qh, ws.eps, ws.thr);
    RC_LAUNCH_CHECK();
}

void run_batched_f8(const BatchPlan &p, BatchWs &ws, hipStream_t s, KernelTimer *timer) {
    const int nq_pad = (p.nq + SB_TILE - 1) / SB_TILE * SB_TILE;
    prepare_queries_f8(p, ws, nq_pad, s);
    auto filter = [&](int64_t c0, int64_t c1, int64_t nchunk, int) {
        launch_filter_f8<false>(p, ws, nq_pad, c0, c1, nchunk, nullptr, s);
    };
    run_stages<f8_t>(p, ws, s, timer, batch_stage_ratio(p.k, ws.cap), p.ld, filter);
}

bool i8_filter_supported(int64_t ld) { return ld == 256 || ld == 512 || ld == 768; }
bool f8_filter_supported(int64_t ld) { return ld == 256 || ld == 512 || ld == 768; }

// rc_index_filter_scores: the float8 filter's own s' (DUMP form of filter_f8_kernel) and eps
void filter_scores_f8(const BatchPlan &p, BatchWs &ws, int64_t row0, int64_t n, float *out_scores, float *out_eps,
                      hipStream_t s) {
    RC_REQUIRE(f8_filter_supported(p.ld), RC_ERR_UNSUPPORTED, "float8 filter needs ld 256, 512 or 768");
    const int nq_pad = (p.nq + SB_TILE - 1) / SB_TILE * SB_TILE;
    prepare_queries_f8(p, ws, nq_pad, s);
    launch_filter_f8<true>(p, ws, nq_pad, row0, row0 + n, 8, out_scores, s);
    RC_LAUNCH_CHECK();
    RC_HIP(hipMemcpyAsync(out_eps, ws.eps, (size_t)p.nq * sizeof(float), hipMemcpyDeviceToDevice, s));
}

void batched_search(const BatchPlan &p, BatchWs &ws, hipStream_t s, KernelTimer *timer) {
    RC_REQUIRE(p.ld % 64 == 0, RC_ERR_UNSUPPORTED, "batched search needs ld % 64 == 0");
    RC_REQUIRE(p.n_rows > 0, RC_ERR_INVALID, "batched search over an empty range");
    if (p.pages != nullptr)  // the int8 and float8 filters have no paged form
        RC_REQUIRE((p.dtype == RC_F16 || p.dtype == RC_BF16) && !p.f8_filter && p.rows8 == nullptr, RC_ERR_UNSUPPORTED,
                   "batched MFMA search over pages needs an f16 or bf16 index with the native or the metric filter");
    if (p.metric != RC_METRIC_COSINE)  // the native kernels' METRIC forms only: the int8 and float8 filters are cosine-only
        RC_REQUIRE((p.dtype == RC_F16 || p.dtype == RC_BF16) && !p.f8_filter && p.rows8 == nullptr && p.norms != nullptr,
                   RC_ERR_UNSUPPORTED, "batched MFMA search under a non-cosine metric needs an f16 or bf16 index with RC_FILTER_METRIC");
    if (p.f8_filter) {
        RC_REQUIRE(p.dtype == RC_F8 && f8_filter_supported(p.ld), RC_ERR_UNSUPPORTED,
                   "float8 filter needs a float8 index of ld 256, 512 or 768");
        return run_batched_f8(p, ws, s, timer);
    }
    if (p.rows8 != nullptr) {
        RC_REQUIRE(i8_filter_supported(p.ld), RC_ERR_UNSUPPORTED, "int8 filter needs ld 256, 512 or 768");
        if (p.dtype == RC_F16 || p.dtype == RC_BF16 || p.dtype == RC_F32)
            return dispatch_dtype(p.dtype, [&](auto t) {  // (no batched search on f8 rows: nothing instantiated)
                if constexpr (!std::is_same_v<decltype(t), f8_t>) run_batched_i8<decltype(t)>(p, ws, s, timer);
            });
    }
    if (p.dtype == RC_F16 || p.dtype == RC_BF16)  // the MFMA operand dtypes
        return dispatch_dtype(p.dtype, [&](auto t) {
            if constexpr (!std::is_same_v<decltype(t), float> && !std::is_same_v<decltype(t), f8_t>) run_batched<decltype(t)>(p, ws, s, timer);
        });
    throw Error(RC_ERR_UNSUPPORTED, "batched MFMA search needs an f16 or bf16 index (or the int8 filter copy)");
}

void BatchWs::ensure(int nq, int k, int64_t ld, int dtype_bytes) {
    const int nq_pad = (nq + SB_TILE - 1) / SB_TILE * SB_TILE;
    if (nq_pad <= nq_cap && k <= k_cap && ld <= ld_cap) return;
    release();
    nq_cap = std::max(nq_pad, 256);
    k_cap = std::max(k, 16);
    ld_cap = ld;
    qn = (float *)dmalloc((size_t)nq_cap * ld * sizeof(float));
    qh = dmalloc((size_t)nq_cap * ld * dtype_bytes);
    eps = (float *)dmalloc((size_t)nq_cap * sizeof(float));
    thr = (float *)dmalloc((size_t)nq_cap * sizeof(float));
    cnt = (uint32_t *)dmalloc((size_t)nq_cap * sizeof(uint32_t));
    cand = (uint32_t *)dmalloc((size_t)nq_cap * cap * sizeof(uint32_t));
    keys = (uint64_t *)dmalloc((size_t)nq_cap * k_cap * sizeof(uint64_t));
    flags = (int *)dmalloc((size_t)nq_cap * sizeof(int));
    sq = (float *)dmalloc((size_t)nq_cap * sizeof(float));
    aq = (float *)dmalloc((size_t)nq_cap * sizeof(float));
    mcoef = (float *)dmalloc((size_t)nq_cap * 4 * sizeof(float));
    ovf = (int *)dmalloc(sizeof(int));
    RC_HIP(hipMemset(ovf, 0, sizeof(int)));
    // the fallback scan's partial lists are sized by a memory budget, not by the row count:
    // 1024 queries x top-100 keep all 256 blocks (210 MB); 4096 x 256 get 32 (268 MB) instead of 2.1 GB
    const int64_t per_block = (int64_t)nq_cap * k_cap * (int64_t)sizeof(uint64_t);
    fb_blocks = (int)std::max<int64_t>(FB_MIN_BLOCKS, std::min<int64_t>(FB_BLOCKS, FB_BUDGET_BYTES / per_block));
    fb_partial = (uint64_t *)dmalloc((size_t)fb_blocks * per_block);
}

void BatchWs::release() {
    for (void *p : {(void *)qn, qh, (void *)eps, (void *)thr, (void *)cnt, (void *)cand, (void *)keys, (void *)flags, (void *)sq,
                    (void *)aq, (void *)mcoef, (void *)ovf, (void *)fb_partial})
        dfree(p);
    *this = BatchWs{};
}

}  // namespace rc

#if defined(RC_GEMM_ABLATION)
// diagnostic builds: the int8 filter's row DMA cache policy (0, or 2 = nontemporal)
extern "C" int rc_diag_set_filter_aux(int aux) {
    return rc::guard([&] {
        RC_REQUIRE(aux == 0 || aux == 2, RC_ERR_INVALID, "aux 0 or 2");
        rc::g_diag_filter_aux = aux;
    });
}
// diagnostic builds: log2 of the bytes of rows per filter sub-launch (31 = the product's 2 GB)
extern "C" int rc_diag_set_filter_split(int log2_bytes) {
    return rc::guard([&] {
        RC_REQUIRE(log2_bytes >= 24 && log2_bytes <= 40, RC_ERR_INVALID, "log2 bytes in [24, 40]");
        rc::g_diag_filter_split_log2 = log2_bytes;
    });
}
#endif
