// index_common.h — what the exact cosine index's translation units share: the storage dtypes,
// the device helpers and in-place macros that carry the search paths' bit-identity (query
// normalisation, the row score's FMA chain, the non-cosine metrics' per-row rule, the int8
// quantisation, the partial-list merge; the wave fold and the output rule are in topk.h), the
// host dispatch over dtype / row width / list size, and the scan's, one-launch query's and
// batched search's argument structs.  The scan's device code is in scan.h.
#pragma once

#include <utility>

#include "rc_common.h"
#include "topk.h"

namespace rc {

struct f16_t { uint16_t b; };
struct bf16_t { uint16_t b; };
// OCP e4m3fn byte of x̂_c · 2⁸ (round to nearest even): the stored value is decode(b) · 2⁻⁸.
// |x̂_c| <= 1, so nothing reaches e4m3's 448, and elements down to 2⁻¹⁴ stay normal.  The scale
// is a power of two, hence exact wherever it is applied: Elem<f8_t>::load applies it to the
// value (fetch, stored rows), the scans fold it into their query registers (F8_UNSCALE at the
// three sites that form them), so unpack16<f8_t> is the bare conversion.
struct f8_t { uint8_t b; };
constexpr float F8_SCALE = 256.0f, F8_UNSCALE = 1.0f / 256.0f;

template <typename T> struct Elem;
template <> struct Elem<float> {
    __device__ static float load(const float *p, int64_t i) { return p[i]; }
    __device__ static float cast(float x) { return x; }
};
template <> struct Elem<f16_t> {
    __device__ static float load(const f16_t *p, int64_t i) { return f16_to_f32(p[i].b); }
    __device__ static f16_t cast(float x) { return f16_t{f32_to_f16(x)}; }
};
template <> struct Elem<bf16_t> {
    __device__ static float load(const bf16_t *p, int64_t i) { return bf16_to_f32(p[i].b); }
    __device__ static bf16_t cast(float x) { return bf16_t{f32_to_bf16(x)}; }
};

template <> struct Elem<f8_t> {
    __device__ static float load(const f8_t *p, int64_t i) { return __builtin_amdgcn_cvt_f32_fp8((int)p[i].b, 0) * F8_UNSCALE; }
    __device__ static f8_t cast(float x) { return f8_t{(uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(x * F8_SCALE, 0.f, 0, false) & 0xff)}; }
};
// What a scan multiplies its query registers by, so that its FMA chain over unpack16's values
// yields the score of the stored values: 1 for every dtype but f8.
template <typename T> constexpr float query_unscale() { return sizeof(T) == 1 ? F8_UNSCALE : 1.0f; }

inline size_t dtype_size(int dtype) { return dtype == RC_F32 ? 4 : dtype == RC_F8 ? 1 : 2; }

// A staging block of stored rows outside any index (row moves between shards, sharded.hip):
// cap rows of ld elements in the storage dtype, and their f32 norms.
struct RowBlock {
    void *rows = nullptr;
    float *norms = nullptr;
    int64_t cap = 0;
};

// unpack one 16-B chunk into its 4 (f32), 8 (f16/bf16) or 16 (f8: decode(b), unscaled) values
template <typename T>
__device__ __forceinline__ void unpack16(const uint4 &x, float *out);
template <>
__device__ __forceinline__ void unpack16<float>(const uint4 &x, float *o) {
    o[0] = __uint_as_float(x.x);
    o[1] = __uint_as_float(x.y);
    o[2] = __uint_as_float(x.z);
    o[3] = __uint_as_float(x.w);
}
template <>
__device__ __forceinline__ void unpack16<f16_t>(const uint4 &x, float *o) {
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o[2 * i] = f16_to_f32((uint16_t)(w[i] & 0xffffu));
        o[2 * i + 1] = f16_to_f32((uint16_t)(w[i] >> 16));
    }
}
template <>
__device__ __forceinline__ void unpack16<bf16_t>(const uint4 &x, float *o) {
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o[2 * i] = __uint_as_float(w[i] << 16);
        o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}

typedef float rc_f32x2 __attribute__((ext_vector_type(2)));
template <>
__device__ __forceinline__ void unpack16<f8_t>(const uint4 &x, float *o) {
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // v_cvt_pk_f32_fp8: two bytes of a word per instruction
        const rc_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
        const rc_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        o[4 * i] = lo.x;
        o[4 * i + 1] = lo.y;
        o[4 * i + 2] = hi.x;
        o[4 * i + 3] = hi.y;
    }
}

// ------------------------------------------------------------ shared device helpers
// Each is the one copy of arithmetic that several kernels must perform alike, bit for bit.

// Query normalisation, one wave (lanes 0..63) per query: 1 / ||src[0, dim)|| (0 for a zero or
// !valid query) from a lane-strided f32 sum of squares, and element c of the normalised,
// zero-padded query (RC_UNIT_ELEM, an expression macro: as a function its load is addressed
// differently in every scan kernel).  Sites: prepare_queries_kernel and prepare_queries_i8_kernel
// (which store the values as qn), scan_rows' raw-query branch and query1_scan (src in LDS), which
// keep them in registers: the same bits everywhere.
// wave_sum_sq is the sum of squares alone (every lane holds the same bits: wave_sum adds
// commutatively in a butterfly) and inv_norm_of the reciprocal norm from it, for the metric
// scans, which need both (metric_coef below).
template <typename P>
__device__ __forceinline__ float wave_sum_sq(P src, int dim, int lane, bool valid = true) {
    float ss = 0.f;
    for (int c = lane; c < dim; c += 64) ss = valid ? fmaf(src[c], src[c], ss) : 0.f;
    return wave_sum(ss);
}
__device__ __forceinline__ float inv_norm_of(float ss) { return ss > 0.f ? 1.0f / sqrtf(ss) : 0.f; }
template <typename P>
__device__ __forceinline__ float wave_inv_norm(P src, int dim, int lane, bool valid = true) {
    return inv_norm_of(wave_sum_sq(src, dim, lane, valid));
}
#define RC_UNIT_ELEM(SRC, C, DIM, INV, VALID) (((VALID) && (C) < (DIM)) ? (SRC)[C] * (INV) : 0.f)

// The non-cosine metrics' per-row rule (rc_index_set_metric; retrieval_core.h states the
// semantics).  A stored row is the direction x̂_r and its f32 norm n = norms[r]; fetch returns
// v_r = x̂_r · n.  With c the row's exact cosine (sum16 of the RC_ROW_FMA16 chain), ss the raw
// query's sum of squares (wave_sum_sq) and qn = sqrtf(ss):
//   dotproduct  q · v_r        = n · (qn · c)                (alpha, beta, gamma) = (qn, 0, 0)
//   euclidean   −‖q − v_r‖²    = n · (2 qn · c − n) − ss                            (2 qn, 1, ss)
// as t = fmaf(alpha, c, −(beta · n)), s = fmaf(n, t, −gamma): one code path, runtime constants.
// s is the top-k key's score and the score returned (descending, so Euclidean distances come
// back negated): the merges and the output rule take it as they take a cosine.  It depends on
// the row and the query alone, so every search path and every sharding give it the same bits.
// Sites: scan_rows_q's metric form (the scan kernels and query1_scan).
struct MetricCoef {
    float alpha, beta, gamma;
};
__device__ __forceinline__ MetricCoef metric_coef(int metric, float ss) {
    // wave-uniform (see wave_sum_sq): kept in scalar registers
    ss = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(ss)));
    const float qn = sqrtf(ss);
    return metric == RC_METRIC_EUCLIDEAN ? MetricCoef{2.0f * qn, 1.0f, ss} : MetricCoef{qn, 0.0f, 0.0f};
}
__device__ __forceinline__ float metric_score(const MetricCoef &m, float c, float n) {
    const float t = fmaf(m.alpha, c, -(m.beta * n));
    return fmaf(n, t, -m.gamma);
}

// Exact row scores take 16 lanes per row: lane sub = lane & 15 holds the row's 16-B chunks
// sub + 16 i (CPL of them, EPC values each) in X[CPL] (uint4) and the same chunks of QB normalised
// queries in Q[QB][CPL][EPC]; RC_ROW_FMA16 sets ACC[b] to the f32 FMA chain in chunk order, and
// the caller's sum16(ACC[b]) is the score.  Sites: scan_rows_q (scan.h) and rescore_kernel
// (search_mfma.hip, QB = 1), hence bit-identical scores on both paths.  (A statement macro: as a
// function taking the register arrays by reference it flips branches in the masked rescore
// kernels and reschedules the multi-query scans.)
template <typename T, int NCH>
struct RowShape {
    static constexpr int EPC = 16 / sizeof(T);           // values per 16-B chunk
    static constexpr int CPL = NCH * 128 / (16 * EPC);   // chunks per lane
    // 16 lanes x CPL chunks cover the row exactly: every NCH but an odd one of f8 rows (16 lanes
    // x 16 B = 256 elements), which no index has (pick_nch) and with_nch does not instantiate
    static constexpr bool WHOLE = CPL * 16 * EPC == NCH * 128;
};
#define RC_ROW_FMA16(T, QB, CPL, EPC, X, Q, ACC)                                                 \
    do {                                                                                         \
        _Pragma("unroll") for (int b_ = 0; b_ < (QB); ++b_) (ACC)[b_] = 0.f;                     \
        _Pragma("unroll") for (int i_ = 0; i_ < (CPL); ++i_) {                                   \
            float f_[EPC];                                                                       \
            unpack16<T>((X)[i_], f_);                                                            \
            _Pragma("unroll") for (int e_ = 0; e_ < (EPC); ++e_)                                 \
                _Pragma("unroll") for (int b_ = 0; b_ < (QB); ++b_)                              \
                    (ACC)[b_] = fmaf(f_[e_], (Q)[b_][i_][e_], (ACC)[b_]);                        \
        }                                                                                        \
    } while (0)

// Symmetric int8 quantisation of a vector v with mx = max |v[c]| (the int8 filter, search_mfma.hip):
// scale = mx / 127, v8[c] = rne(v[c] / scale) clamped to [-127, 127], and from the f32 sum of
// squares ss of v - scale·v8 the bound >= ||v - scale·v8||₂ (x1.001 covers the f32 sum, +1e-7 the
// f32 residuals).  Stored rows (quantize_rows_kernel) and queries (prepare_queries_i8_kernel) both
// use these: the filter bound's proof needs the two sides rounded alike.
__device__ __forceinline__ float i8_scale(float mx) { return mx * (1.0f / 127.0f); }
__device__ __forceinline__ float i8_inv_scale(float mx) { return mx > 0.f ? 127.0f / mx : 0.f; }
__device__ __forceinline__ float i8_round(float x, float inv_scale) { return fminf(127.f, fmaxf(-127.f, rintf(x * inv_scale))); }
__device__ __forceinline__ float i8_resid_bound(float ss) { return sqrtf(ss) * 1.001f + 1e-7f; }

// ----------------------------------------------------------------- host dispatch
// Each calls f with a type tag / std::integral_constant for the runtime value, from a generic
// lambda (as gemm.h's with_k_tiles), so a launch site names its kernel once.
template <typename F>
void dispatch_dtype(int dtype, F &&f) {
    switch (dtype) {
        case RC_F32: f(float{}); break;
        case RC_F16: f(f16_t{}); break;
        case RC_BF16: f(bf16_t{}); break;
        case RC_F8: f(f8_t{}); break;
        default: throw Error(RC_ERR_INVALID, "unknown dtype");
    }
}

inline int topk_cap(int k) {
    int kp = 16;
    while (kp < k) kp <<= 1;
    return kp * 2 < 128 ? 128 : kp * 2;
}

// f(integral_constant<CAP>) for the WaveTopK list size CAP in {128, 256, 512} that holds
// cap = topk_cap(k); false (f not called, nor instantiated) if that is beyond MAX_CAP.
template <int MAX_CAP = 512, typename F>
bool with_topk_cap(int cap, F &&f) {
    if (cap <= 128) return f(std::integral_constant<int, 128>{}), true;
    if constexpr (MAX_CAP >= 256) {
        if (cap <= 256) return f(std::integral_constant<int, 256>{}), true;
    }
    if constexpr (MAX_CAP >= 512) return f(std::integral_constant<int, 512>{}), true;
    return false;
}

// f(integral_constant<NCH>) for the row width ld = 128 * nch, nch in {1, 2, 3, 4, 6, 8, 12, 16}
// up to MAX_NCH that rows of T can have (RowShape::WHOLE: the even ones for f8); false (f not
// called, nor instantiated) for any other.
template <int MAX_NCH, typename T, typename F, int... N>
bool with_nch_of(int nch, F &&f, std::integer_sequence<int, N...>) {
    auto one = [&](auto n) {
        if constexpr (decltype(n)::value <= MAX_NCH && RowShape<T, decltype(n)::value>::WHOLE) {
            if (nch == decltype(n)::value) return f(n), true;
        }
        return false;
    };
    return (one(std::integral_constant<int, N>{}) || ...);
}
template <int MAX_NCH = 16, typename T = float, typename F>
bool with_nch(int nch, F &&f) {
    return with_nch_of<MAX_NCH, T>(nch, f, std::integer_sequence<int, 1, 2, 3, 4, 6, 8, 12, 16>{});
}

struct ScanArgs {
    const void *rows;
    int64_t ld;
    int nch;
    int64_t n_rows;
    int64_t rows_per_block;
    int nblk;
    const float *qn;
    int q0;
    int qb;
    int nq_total;
    int k;
    uint64_t *partial;
    hipStream_t stream;
    // Exact fallback of the batched search: when set, grid.y strides over the
    // queries [0, nq_total) and only queries with flags[q] != 0 are scanned
    // (qb = 1; q0 unused); partial is then [nblk][nq_total][k].
    const int *flags = nullptr;
    int grid_y = 1;
    // Single-query scans (scan_search): the raw queries [nq_real][dim]; every wave normalises its
    // query itself (wave_inv_norm / RC_UNIT_ELEM: no separate launch), and qn is not read.
    // nullptr: qn holds the normalised queries.
    const float *qraw = nullptr;
    int dim = 0, nq_real = 0;
    // Row-masked scan (rc_index_search_masked): device bitmap over the local rows, bit r & 31 of
    // word r >> 5 = row r is eligible, ceil(n_rows / 32) words (bits at or past n_rows are not
    // trusted).  nullptr: every row is eligible (the unmasked kernels; no runtime test of it on
    // the device, the host picks the instantiation).
    const uint32_t *mask = nullptr;
    // Scoring rule (rc_index_set_metric).  Not RC_METRIC_COSINE: the metric kernels
    // (launch_scan_metric), which read norms [n_rows] and need raw queries (qraw), one per pass
    // (qb = 1).  With flags (f16 / bf16 rows only): the metric batched search's exact fallback,
    // grid.y striding over the flagged queries as above, each normalised from qraw.
    int metric = RC_METRIC_COSINE;
    const float *norms = nullptr;
};

// largest queries-per-pass for a row width: query registers per lane = QB*nch*8 floats <= 64
// (the masked scan is instantiated for multi-query passes at the smallest list size only, the
// metric scans for single-query passes only)
inline int scan_max_qb(int nch, int k, bool masked = false, int metric = RC_METRIC_COSINE) {
    if (metric != RC_METRIC_COSINE) return 1;
    if (k > (masked ? 64 : 128)) return 1;
    return nch <= 2 ? 4 : (nch <= 4 ? 2 : 1);
}

template <typename T>
void launch_scan(const ScanArgs &a);  // scan.h; instantiated in scan_{f32,f16,bf16,f8}.hip
template <typename T>
void launch_scan_metric(const ScanArgs &a);  // scan_metric.h; instantiated in scan_metric_{f32,f16,bf16,f8}.hip

// One query, one launch (rc_sharded_query_host's request path): query1_kernel normalises the
// query (carried in the kernel arguments: no copy), scans its block's rows, and the last block
// to finish merges every block's partial list and gathers the matched rows' values, writing
// scores / rows / values straight into (host-mapped) output memory.
constexpr int QUERY1_MAX_DIM = 768;       // the query rides in the kernarg segment (< 4 KB); a multiple of 256
constexpr int QUERY1_MAX_BLOCKS = 256;    // partial lists the last block merges, at most
constexpr int64_t QUERY1_MAX_ROWS = 1 << 20;  // beyond this the multi-kernel scan has more blocks in flight
struct Query1Args {
    const void *rows;
    const float *norms;
    int64_t ld;
    int dim;
    int nch;
    int64_t n_rows;
    int64_t rows_per_block;
    int nblk;
    int k;
    int with_values;
    int metric;             // RC_METRIC_*; sits in what was padding: the cosine kernels' argument layout is unchanged
    int64_t row_base, row_stride;
    uint64_t *partial;      // [nblk][k]
    float *out_scores;      // [k]
    int64_t *out_rows;      // [k]
    float *out_values;      // [k][dim] (with_values)
    unsigned *done;         // optional host-coherent word: the finishing block stores seq there last
    unsigned seq;
    float q[QUERY1_MAX_DIM];
};
static_assert(sizeof(Query1Args) == 3200, "Query1Args is the one-launch kernels' argument block");
template <typename T>
void launch_query1(const Query1Args &a, hipStream_t s);  // scan.h; instantiated in scan_{f32,f16,bf16,f8}.hip
// phase 1 under a non-cosine metric (launch_query1 calls it); scan_metric.h, instantiated in scan_metric_{f32,f16,bf16,f8}.hip
template <typename T>
void launch_query1_metric_scan(const Query1Args &a, hipStream_t s);

// Merge nlist sorted partial lists of k keys (query qi of nq_total) into wave 0's tk: the body
// of merge_partials_kernel, shared with query1_kernel's last block.  Block-collective.
template <int CAP>
__device__ __forceinline__ void merge_partial_lists(const uint64_t *__restrict__ partial, int nlist, int nq_total, int qi, int k,
                                                    uint64_t (&lds)[4][CAP], WaveTopK<CAP> &tk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    tk.init(as_lds(&lds[wave][0]), k);
    const int64_t total = (int64_t)nlist * k;
    // MERGE_U independent loads in flight per lane before any is consumed: the
    // loop is latency-bound otherwise (one dependent HBM/L2 round trip per 64 keys)
    constexpr int MERGE_U = 8;
    for (int64_t j0 = (int64_t)wave * 64 * MERGE_U; j0 < total; j0 += 256 * MERGE_U) {
        uint64_t key[MERGE_U];
#pragma unroll
        for (int u = 0; u < MERGE_U; ++u) {
            const int64_t j = j0 + u * 64 + lane;
            key[u] = KEY_EMPTY;
            if (j < total) {
                const int64_t l = j / k, t = j - l * k;
                key[u] = partial[(l * nq_total + qi) * k + t];
            }
        }
#pragma unroll
        for (int u = 0; u < MERGE_U; ++u) {
            tk.reserve(64);
            tk.push(key[u] != KEY_EMPTY, key[u]);
        }
    }
    tk.compact();
    __syncthreads();
    if (wave == 0) fold_wave_lists<CAP>(&lds[0][0], CAP, tk, k);
}

// ------------------------------------------- batched MFMA search (search_mfma.hip)
constexpr int BATCH_CAND_CAP = 4096;  // candidate slots per query per stage
constexpr int INDEX_ROW_PAD = 256;    // row storage is allocated in whole 256-row tiles
constexpr int FB_BLOCKS = 256;        // blocks of the on-device exact fallback scan (overflowed queries), at most
constexpr int FB_MIN_BLOCKS = 32;     // ... and at least, whatever the memory budget below says
constexpr int64_t FB_BUDGET_BYTES = int64_t(256) << 20;  // cap on its partial-key buffer per index
constexpr int FB_QSTRIDE = 64;        // its grid.y: block (b, y) scans queries y, y + 64, ... that overflowed

struct BatchWs {
    int nq_cap = 0, k_cap = 0;
    int64_t ld_cap = 0;
    int cap = BATCH_CAND_CAP;
    float *qn = nullptr;        // [nq_cap][ld] normalised queries (f32)
    void *qh = nullptr;         // [nq_cap][ld] queries in the storage dtype (MFMA operand); float8: two byte planes
    float *eps = nullptr;       // [nq_cap] bound on |s' - s|
    float *thr = nullptr;       // [nq_cap] current filter threshold
    uint32_t *cnt = nullptr;    // [nq_cap] candidates appended this stage
    uint32_t *cand = nullptr;   // [nq_cap][cap] candidate rows
    uint64_t *keys = nullptr;   // [nq_cap][k_cap] running top-k keys (sorted)
    int *flags = nullptr;       // [nq_cap] 1 = candidate overflow, exact fallback needed
    float *sq = nullptr;        // [nq_cap] int8 filter: query scale (q̃ = sq · q8)
    float *aq = nullptr;        // [nq_cap] int8 filter: coefficient of a row's residual norm in the bound
    float *mcoef = nullptr;     // [nq_cap][4] metric filter: (eps, alpha, beta, gamma) of each query (metric_coef)
    int *ovf = nullptr;         // overflowed queries since the last timing read (device counter)
    int fb_blocks = 0;               // blocks of the fallback scan: FB_BUDGET_BYTES / (nq_cap * k_cap * 8), clamped
    uint64_t *fb_partial = nullptr;  // [fb_blocks][nq_cap][k_cap] partial keys of the exact fallback scan
    void ensure(int nq, int k, int64_t ld, int dtype_bytes);
    void release();
};

struct BatchPlan {
    const void *rows;
    int dtype;
    int dim;
    int nch;
    int64_t ld;
    int64_t n_rows;
    int64_t row_base;      // returned row = row_base + local row * row_stride
    int64_t row_stride;
    const float *queries;  // device f32 [nq][dim]
    int nq;
    int k;
    float *out_scores;
    int64_t *out_rows;
    // int8 filter copy of the rows (rc_index_set_filter(RC_FILTER_I8)), or null
    const int8_t *rows8 = nullptr;  // [cap_pad][ld] x8, x̃ = sx · x8
    const float *rsx = nullptr;     // [cap_pad] sx, at i8_slot(row)
    const float *rex = nullptr;     // [cap_pad] ||x̂ - x̃||₂ (rounded up), at i8_slot(row)
    // row-eligibility bitmap over the local rows (ScanArgs::mask), or null: applied in rescore_kernel
    const uint32_t *mask = nullptr;
    // RC_SEARCH_MFMA_MASKED (mask != null): the filter kernels' MASKED forms apply the bitmap too
    bool mask_filter = false;
    // float8 index with rc_index_set_filter(RC_FILTER_F8): the filter GEMM reads the stored e4m3 rows
    bool f8_filter = false;
    // RC_FILTER_METRIC under a non-cosine metric: the native filter kernels' metric forms, which
    // bound each row's metric score and read norms [n_rows]; the keys carry metric scores
    int metric = RC_METRIC_COSINE;
    const float *norms = nullptr;
    // a slot's page table (rc_index_search_pages_ex), or null: n_rows, the mask, the candidates and
    // the returned rows are then POSITIONS of that table, and the kernels are the PAGED forms
    // (search_mfma_paged.hip; f16 / bf16 rows, native or metric filter)
    const int32_t *pages = nullptr;
};

// The int8 filter keeps a row's scale and residual norm at a tile-transposed slot:
// within each 128-row tile, row 16·rf + li sits at 8·li + rf, so the filter lane that
// holds rows {16·rf + li : rf} reads its 8 values as two 16-B loads.
__host__ __device__ __forceinline__ int64_t i8_slot(int64_t row) {
    return (row & ~int64_t(127)) + (row & 15) * 8 + ((row & 127) >> 4);
}
bool i8_filter_supported(int64_t ld);  // row widths filter_i8_kernel is instantiated for
bool f8_filter_supported(int64_t ld);  // ... and filter_f8_kernel
// the paged native filter kernels (search_mfma_paged.hip): every form but ld 512 with METRIC and MASKED
bool paged_filter_supported(int64_t ld, bool metric, bool mask_filter);

// Enqueue the staged filter-GEMM / rescore search on `s` (no host sync).
void batched_search(const BatchPlan &p, BatchWs &ws, hipStream_t s, KernelTimer *timer);
int batch_stage_ratio(int k, int cap, int inflation = 1);
// The float8 filter's scores s' of p.queries against local rows [row0, row0 + n) (row0 a multiple
// of 128), f32 [nq][n], and its eps [nq], enqueued on `s` (rc_index_filter_scores).
void filter_scores_f8(const BatchPlan &p, BatchWs &ws, int64_t row0, int64_t n, float *out_scores, float *out_eps,
                      hipStream_t s);

}  // namespace rc
