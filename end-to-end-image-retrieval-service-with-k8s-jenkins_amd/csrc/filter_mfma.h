// filter_mfma.h — what the batched search's native (f16 / bf16) filter kernels share between their
// two translation units: search_mfma.hip (the contiguous kernels and every host function) and
// search_mfma_paged.hip (the page-table forms of the same bodies).  The MFMA wrappers, the filter
// arguments, the block mapping, the candidate append, and the MASKED and METRIC epilogues' helpers
// with the arguments that make them exact.  The kernel bodies themselves are filter_gemm_body.inc
// and filter_qs_body.inc.
#pragma once

#include "index_common.h"

namespace rc {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

template <typename T> struct MfmaOp;
template <> struct MfmaOp<f16_t> {
    typedef _Float16 v8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ f32x4_t mma(v8 a, v8 b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};
template <> struct MfmaOp<bf16_t> {
    typedef __bf16 v8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ f32x4_t mma(v8 a, v8 b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

constexpr int SB_TILE = 256;  // queries per query block = rows per row tile

// ------------------------------------------------------- filter GEMM -------
struct FilterArgs {
    const void *rows;  // [>= roundup(r_end, 256)][ld]
    const void *qh;    // [nqb*256][ld]
    int64_t ld;
    int nkt;           // ld / 64
    int64_t r_begin;   // multiple of 256
    int64_t r_end;
    int64_t tiles_per_chunk;
    int nqb;
    const float *thr;  // [nqb*256]
    uint32_t *cnt;     // [nqb*256]
    uint32_t *cand;    // [nqb*256][cap]
    int cap;
    // int8 filter only (filter_i8_kernel): per-row sx / ex at i8_slot(row), per-query sq / aq
    const float *rsx = nullptr, *rex = nullptr, *sq = nullptr, *aq = nullptr;
};

// Block → (query block, row chunk), for tiles of RT rows: blocks b and b+8 share an XCD; the nqb
// blocks of one chunk are consecutive on one XCD, so each row tile is read from HBM once and
// served to the other query blocks from that XCD's L2.  The block's row tiles are [rt0, rt1)
// (none: rt0 >= rt1, a block-uniform early return for the caller).
struct FilterBlock {
    int qb;
    int64_t rt0, rt1;
    __device__ __forceinline__ FilterBlock(const FilterArgs &a, int RT) {
        const int b = blockIdx.x, xcd = b & 7, jx = b >> 3;
        qb = jx % a.nqb;
        const int64_t chunk = (int64_t)(jx / a.nqb) * 8 + xcd;
        const int64_t rt_total = (a.r_end - a.r_begin + RT - 1) / RT;
        rt0 = chunk * a.tiles_per_chunk;
        rt1 = min(rt_total, rt0 + a.tiles_per_chunk);
    }
};

// Row `row` passed query q's filter: append it to q's candidate list (the count keeps running
// past cap: rescore_kernel reads an overflow from it).
__device__ __forceinline__ void append_candidate(const FilterArgs &a, int q, int64_t row) {
    const uint32_t pos = atomicAdd(&a.cnt[q], 1u);
    if ((int)pos < a.cap) a.cand[(int64_t)q * a.cap + pos] = (uint32_t)row;
}

// -------------------------------------- MASKED epilogues (RC_SEARCH_MFMA_MASKED) --
// Every filter kernel has a MASKED form (a compile-time form, as scan_rows_q's and rescore_kernel's:
// the unmasked kernels keep their instructions).  It reads the row-eligibility bitmap over the LOCAL
// rows that rescore_kernel<.., MASKED> reads (bit r & 31 of word r >> 5) and appends (q, row) iff
// the kernel's own test passes AND the row's bit is set.
// Why it stays exact: the unmasked argument (the header's, the metric epilogue's, the int8 and float8
// bounds) restricted to the eligible rows.  The result is the top-k of the eligible rows.  thr[q] comes
// from rescore_kernel, which under a mask merges eligible rows only: it is the k-th best exact score
// of the ELIGIBLE rows seen so far (minus eps[q]; -inf while fewer than k were seen), a lower bound of
// the final k-th best eligible score, and it only rises.  An eligible row of the final top-k therefore
// passes the kernel's test at its stage as before, and its bit is set: it is appended.  Ineligible
// rows were never part of the result; leaving them out only shortens the lists, so a stage collects
// ≈ k·(g - 1) candidates whatever the eligible share, where the unmasked filter under a mask collects
// 1 / share times as many ("Masked search").  A clustered mask can still overflow a
// stage: the flagged queries take the masked scan on the device, as before.
// A row tile starts at a multiple of 64 rows, so its bits are whole words at a wave-uniform address:
// scalar loads into scalar registers, issued a tile (or a K loop) ahead of the epilogue that reads
// them.  A tile without an eligible row skips its epilogue on a wave-uniform branch (its loads and
// MFMAs stay: they are one flattened pipeline).
//
// NW words of the 32·NW rows from `first_row` (a multiple of 64).  The bitmap holds ceil(r_end / 32)
// words and the last tile reaches past r_end: the index is clamped to the last word (a read past the
// bitmap is a fault) and a word wholly past r_end reads as 0.  Bits at or past r_end inside the last
// word may be set: the epilogues keep their row < r_end test.
template <int NW>
__device__ __forceinline__ void load_mask_words(const uint32_t *__restrict__ mask, int64_t first_row, int64_t r_end,
                                                uint32_t (&w)[NW]) {
    // Through the constant address space (the bitmap does not change while a search runs): only
    // there does the compiler load a uniform address with the scalar unit.  As a global load the
    // words were vector registers held across the K loop, and the NKT 8 forms spilled.
    typedef const __attribute__((address_space(4))) uint32_t *const_words;
    const const_words cm = (const_words)mask;
    const int64_t w0 = first_row >> 5, wl = (r_end - 1) >> 5;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const uint32_t v = cm[min(w0 + i, wl)];
        w[i] = w0 + i <= wl ? v : 0u;
    }
}
// A lane's four consecutive rows of one f32 accumulator, their eligibility in bits 0-3 of e: the
// ineligible ones become NaN ahead of the epilogue's maximum, so both levels of its early-out see
// eligible rows only.  NaN and not -inf: while thr[q] is still -inf, -inf >= thr holds and the row
// would be appended; NaN fails every >=, and fmaxf returns its other operand, so the maximum runs
// over the eligible rows (-inf when the lane has none).
__device__ __forceinline__ f32x4_t mask_ineligible4(f32x4_t v, uint32_t e) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (e >> j) & 1u ? v[j] : __builtin_nanf("");
    return v;
}

// ---------------------------------------- metric epilogue (RC_FILTER_METRIC) --
// Under dotproduct / euclidean the two native filter kernels have a METRIC form: the same
// GEMM, and an epilogue that bounds the row's METRIC score instead of testing the cosine.  (The
// int8 and float8 filters have no such form: they stay cosine-only.)
//
// s' is the filter GEMM's accumulator for (query q, row r), c the exact cosine the scan and
// rescore_kernel compute in f32 (RC_ROW_FMA16 + sum16), and |s' - c| <= eps[q] (the header's
// bound, prepare_queries_kernel's eps).  With n = norms[r] and (alpha, beta, gamma) the query's
// metric_coef constants, the filter keeps (q, r) iff
//     u = metric_score(mc, ĉ, n) >= thr[q],     ĉ = s' + eps[q]   (one f32 add)
// where under a metric thr[q] is the running k-th best EXACT metric score itself (-inf until k
// rows are held), with no eps subtracted (rescore_candidates).
// Exact, because u >= the row's exact score s = metric_score(mc, c, n), bit for bit:
//   * ĉ >= c.  The real number s' + eps is >= c; rounding to nearest is monotone and c is an f32,
//     so fl(s' + eps) >= fl(c) = c: the add's rounding cannot take ĉ below c.
//   * t(x) = fmaf(alpha, x, -(beta·n)) is non-decreasing in x for alpha >= 0 (alpha is ‖q‖ or
//     2‖q‖): the exact alpha·x - fl(beta·n) is, and a correctly rounded FMA is a monotone
//     function of its exact value.  The addend fl(beta·n) is the same f32 on both sides.
//   * s(t) = fmaf(n, t, -gamma) is non-decreasing in t for n >= 0 (a norm), likewise.
//   So ĉ >= c gives u = s(t(ĉ)) >= s(t(c)) = s: no second slack term.  The running k-th best only
//   rises, so every row of the final top-k has s >= thr[q] at its stage, hence u >= thr[q]; rows
//   tied with the k-th score pass because the test is >=.
// The per-row arithmetic is metric_score itself (one copy, index_common.h), so the three roundings
// are the scan's.  In these epilogues a lane owns one query and four consecutive rows per
// accumulator: the constants are per lane, loaded as prepared (metric_coef assumes a wave-uniform
// query and is not called here), and a lane's four norms are one aligned 16-byte load.
// norms holds `capacity` floats, not the padded row count, and the last row tile reaches past
// r_end: the norm index is clamped to r_end - 1 (as the metric scan loads its norms under the
// rows' clamp).  A row >= r_end then gets some u, which can only defeat the wave-uniform
// early-out: the append still tests row < r_end.
// The epilogues overwrite the accumulators with u and then run the cosine epilogue's own test on
// them (the maximum of u as the wave-uniform early-out, then u >= thr per row): no second copy of
// the tile in registers.  The norm loads sit in the epilogue itself, so each tile's epilogue waits
// for the row DMA in flight before it (vector-memory loads return in order); DESIGN.md, "Metric
// filter", has what that costs against the cosine launch.
struct FilterMetric {
    const float *norms;  // [>= r_end]
    const float *mcoef;  // [nqb*256][4]: eps, alpha, beta, gamma
};

// norms of a row tile's rows o .. o + 3 (o a multiple of 4): tn = the norm of the tile's first row
// (wave-uniform), left >= 1 = how many of the tile's rows are below r_end; indices clamped to
// left - 1.  Offsets in 32 bits against the uniform base: one address register per load.
__device__ __forceinline__ f32x4_t load_norms4(const float *__restrict__ tn, int o, int left) {
    if (o + 4 <= left) return *reinterpret_cast<const f32x4_t *>(tn + o);
    f32x4_t v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = tn[min(o + j, left - 1)];
    return v;
}
// u of the comment above: k4 =(eps, alpha, beta, gamma) of the lane's query
__device__ __forceinline__ float metric_upper(const f32x4_t &k4, float sp, float n) {
    return metric_score(MetricCoef{k4[1], k4[2], k4[3]}, sp + k4[0], n);
}

// filter_qs_kernel's shape (search_mfma.hip): queries/16 per wave, rows per tile, LDS ring steps
constexpr int QS_QT = 2, QS_RT = 128, QS_NS = 8;

// ------------------------------------------------ PAGED forms (search_mfma_paged.hip) --
// Both bodies have a PAGED form (`constexpr bool PAGED`, `const int32_t *pages`): the rows are a
// namespace's positions [r_begin, r_end) of a page table (scan_paged.h), and everything but two
// addresses stays in position space.  A row tile is SB_TILE or QS_RT positions from a multiple of
// its own size, and every stage and sub-launch boundary of run_stages is a multiple of SB_TILE, so a
// tile lies inside one page: its local row is pages[pos >> 8] · 256 + (pos & 255).
static_assert(RC_PAGE_ROWS == SB_TILE && RC_PAGE_ROWS % QS_RT == 0 && BATCH_CAND_CAP % RC_PAGE_ROWS == 0,
              "a row tile of either filter kernel never straddles two pages");
// The page of position `pos` (pos < r_end <= n_pos: inside the table).  One wave-uniform word,
// through the constant address space as load_mask_words' words and for its reason: a scalar load
// into a scalar register, none of the lane's own.
__device__ __forceinline__ int32_t load_page(const int32_t *__restrict__ pages, int64_t pos) {
    typedef const __attribute__((address_space(4))) int32_t *const_pages;
    return ((const_pages)pages)[pos / RC_PAGE_ROWS];
}
// One filter dispatch over a page table (search_mfma_paged.hip, instantiated for f16 / bf16): fa as
// run_batched fills it, in positions.
template <typename T>
void launch_filter_paged(const BatchPlan &p, const BatchWs &ws, FilterArgs fa, int64_t nchunk, int nqb, hipStream_t s);
// what a contiguous kernel declares ahead of the body in place of the paged form's argument
#define RC_FILTER_NOT_PAGED         \
    constexpr bool PAGED = false; \
    [[maybe_unused]] const int32_t *const pages = nullptr;

}  // namespace rc
