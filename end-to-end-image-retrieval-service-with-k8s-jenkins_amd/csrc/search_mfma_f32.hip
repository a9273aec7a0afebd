// search_mfma_f32.hip — the float32 filter (rc_index_set_filter(RC_FILTER_F32)): the batched
// search's filter GEMM over the stored rows of a FLOAT32 index, with no copy of them.
//
// gfx950 has no f32-input MFMA worth using (the xf32 forms are gone), and the filter needs none:
// it only has to bound the exact score from above, and rescore_kernel rescores f32 rows exactly
// (it already does for the int8 filter on an f32 index).  So filter_f32_kernel streams the stored
// f32 rows, narrows each fragment to f16 in registers on its way to v_mfma_f32_16x16x32_f16, and
// prepare_queries_f32_kernel puts the narrowing into the bound.  Everything after the filter is
// what the other filters use: rescore_kernel<float> under cosine, launch_rescore_metric<float>
// (rescore_metric_f32.hip) under dotproduct / euclidean, the f32 scan or metric scan as the
// overflow fallback.
//
// The kernel.  Query-stationary, as filter_qs_kernel / filter_f8_kernel: the FilterBlock mapping,
// 8 waves (2 per SIMD), an LDS ring filled by buffer-descriptor LDS-DMA (uniform base, 32-bit lane
// offsets), every ring step issued (past the block's range through a zero-size descriptor) so that
// each wait counts a fixed number of younger loads.  What is its own:
//   * Queries.  A wave holds 16·QT queries for the whole launch as NKS = ld / 32 f16 B-fragments
//     of 4 VGPRs per query tile: lane (li, g) has columns [32 ks + 8 g, + 8) of query q0 + 16 qt +
//     li, read once from the f16 operand prepare_queries_f32_kernel wrote.
//   * Rows.  One ring step is one MFMA K: 32 columns x RT rows of f32 = RT x 128 bytes (16 KB at
//     RT 128, the f16 kernel's step).  Lane (li, g)'s A-fragment of row group rf is the 8
//     consecutive f32 [32 ks + 8 g, + 8) of row 16 rf + li: the 16-byte chunks 2g and 2g + 1 of
//     the row's 128 bytes, two ds_read_b128, then four v_cvt_pk_f16_f32 (what hipcc emits for the
//     __builtin_convertvector below: round to nearest even under the kernel's default mode) into
//     the 4 VGPRs of the MFMA's A operand.  The f32 staging is GF = 2 fragments of 8 VGPRs, rolling
//     as in filter_f8_kernel: fragment f + GF is read into fragment f's slot once f is converted
//     and its QT MFMAs have issued.
//   * LDS layout and bank conflicts.  A row's K-step is 128 bytes = 32 banks of the 64, so rows r
//     and r + 2 start on the same bank, and a quarter-wave's fragment read (16 lanes of one g:
//     rows li = 0..15, the same chunk 2g + h of each) would put 16 x 16 bytes on the 8 banks of
//     that chunk and its neighbour row's: an 8-way conflict.  Swizzled as the other ring kernels:
//     chunk c of row r sits at position c ^ ((r >> 1) & 7) of the row's 128 bytes (the DMA lane
//     that writes position p of row r loads chunk p ^ ((r >> 1) & 7) from global memory; (r >> 1)
//     & 7 = (li >> 1) & 7 for r = 16 rf + li, whatever rf).  The read of chunk 2g + h by lane li
//     then starts at bank 32·(li & 1) + 4·((2g + h) ^ (li >> 1)): li >> 1 takes 8 values, so the
//     XOR takes 8 distinct positions in each half of the banks, and the 16 lanes cover all 64
//     banks exactly once.  No conflict, for either chunk; no padding, so the DMA stays whole
//     1 KB pieces (8 rows x 128 B per wave instruction).
//   * MFMA roles as filter_qs_kernel (A = index rows, B = queries): lane (li, g) of acc[rf][qt]
//     holds rows 16 rf + 4 g + j of query 16 qt + li, so append_candidate, load_mask_words /
//     mask_ineligible4, load_norms4 / metric_upper and FilterBlock (filter_mfma.h) apply as they are.
//   * METRIC, MASKED and DUMP are compile-time forms.  METRIC: the metric epilogue of filter_mfma.h
//     (u = metric_score at s' + eps, against the running k-th best metric score).  DUMP
//     (rc_index_filter_scores): the epilogue stores s' instead of testing it.
// Shapes (registers: 256 per lane at 2 waves per SIMD; query fragments 4·QT·NKS, accumulators
// RT/16·QT·4, f32 staging 16 + 4 converted; VGPRs of the cosine form ... the METRIC MASKED form):
//   ld 128: NKS  4, QT 2, RT 128:  32 + 64, 140 ... 251
//   ld 256: NKS  8, QT 2, RT  64:  64 + 32, 136 ... 188 (RT 128: the METRIC forms spill 12 and 68 bytes)
//   ld 512: NKS 16, QT 2, RT  64: 128 + 32, 256
//   ld 768: NKS 24, QT 1, RT  64:  96 + 16, 147 ... 191 (QT 2 would hold 192 in query fragments alone:
//           a block is 128 queries there, and a row-fragment read and conversion feeds 1 MFMA instead of 2)
// No instantiation uses scratch (profiles/f32_filter/kernel_resources.txt).  The ring is 8 steps
// of 128 rows or 16 of 64: 128 KB.
//
// The bound.  c is the exact f32 cosine the scan and rescore_kernel compute for (query q, stored
// row x), qn the normalised f32 query, q̂ = f16(qn) the B operand, x̃ = f16(x) the A operand, s'
// the accumulator.  Then
//     |s' - c| <= |q̂·x̃ - qn·x| + A + B,   q̂·x̃ - qn·x = (q̂ - qn)·x + q̂·(x̃ - x)
//     |s' - c| <= ‖qn - q̂‖·‖x‖ + ‖q̂‖·‖x̃ - x‖ + A + B
// with A, B the f32 accumulation errors of s' and of c.  Term by term:
//   * ‖x‖ <= 1.01 (a stored row is normalised in f32), and ‖qn - q̂‖ is computed: the first term
//     is prepare_queries_kernel's 1.01·√err.
//   * The row narrowing, the term the other filters do not have.  v_cvt_pk_f16_f32 rounds to
//     nearest even; |x_i| <= 1.01 never overflows.  For |x_i| >= 2⁻¹⁴ (f16's normal range)
//     |x̃_i - x_i| <= 2⁻¹¹·|x_i|; below it the result is a multiple of 2⁻²⁴ and |x̃_i - x_i| <=
//     2⁻²⁵.  Hence ‖x̃ - x‖ <= 2⁻¹¹·‖x‖ + √ld·2⁻²⁵ <= 1.01·2⁻¹¹ + √ld·2⁻²⁵ =: ρ(ld) (4.94e-4 at
//     ld 768), and the term is ‖q̂‖·ρ(ld) with ‖q̂‖ computed from the f16 values themselves.
//     (Another conversion would need another constant: a round-toward-zero pack doubles the
//     relative part, bf16 makes it 2⁻⁹.  F32F_ROW_REL / F32F_ROW_ABS are this instruction's.)
//     ASSUMPTION: f16 values below 2⁻¹⁴ are kept, by the conversion (the kernel's default
//     float mode keeps f16 denormals) and by the MFMA (from CDNA3 on the f16 MFMAs do not flush
//     their inputs; CDNA2 did).  Flushed, the absolute part would be 2⁻¹⁴ per element.
//     tests/test_f32_filter_gpu.py measures |s' - c₆₄| <= eps through rc_index_filter_scores on
//     rows whose tails sit in that range, with a query aligned to such a tail.
//   * A + B: each at most ld·2⁻²⁴·‖·‖‖·‖ (an f32 chain of ld products; for the MFMA's internal
//     order the same truncation model as the float8 filter's c_mfma): 6.5e-5 covers both up to ld
//     512, as in prepare_queries_kernel, and is scaled by ld / 512 above it.
// eps[q] = (1.01·‖qn - q̂‖ + ‖q̂‖·ρ(ld) + A + B), norms rounded up as i8_resid_bound does, the sum
// by 1.0001: ≈ 8e-4 for a unit query at ld 768 (‖qn - q̂‖ ≈ 2e-4), three to four times the native
// f16 filter's and a tenth of the int8 filter's.  Why the filter is exact with it: the header of
// search_mfma.hip, unchanged.  Under a metric eps goes into mcoef[q][0], so ĉ = s' + eps >= c and
// metric_upper's argument (filter_mfma.h) holds as it stands.
// Candidate growth: the lists grow by exp(z·Δeps / σ) over the f16 filter's; for random unit
// rows at ld 768 (σ = 0.036, z = 3.7 at top-100 of 1M, Δeps ≈ 5e-4) that is 1.05: no stage
// inflation (batch_stage_ratio's default).  An estimate from the formula, not a measurement.
#include "filter_mfma.h"
#include "index_common.h"

namespace rc {

constexpr float F32F_ROW_REL = 1.0f / 2048.0f;      // 2⁻¹¹: half an ulp of a normal f16, relative
constexpr float F32F_ROW_ABS = 1.0f / 33554432.0f;  // 2⁻²⁵: half the spacing of f16 below 2⁻¹⁴
constexpr float F32F_ROW_NORM_MAX = 1.01f;

// Queries: qn exactly as prepare_queries_kernel / prepare_queries_metric_kernel form it (the
// rescored bits stay the scan's), qh = f16(qn), eps (the header's bound) and thr; METRIC: mcoef =
// (eps, alpha, beta, gamma) with metric_coef on the metric scan's own sum of squares.
template <bool METRIC>
__global__ __launch_bounds__(64) void prepare_queries_f32_kernel(const float *__restrict__ q, int nq, int dim, int64_t ld,
                                                                int metric, float *__restrict__ qn, f16_t *__restrict__ qh,
                                                                float *__restrict__ eps, float *__restrict__ thr,
                                                                float *__restrict__ mcoef) {
    const int lane = threadIdx.x;
    const int qi = blockIdx.x;
    const bool valid = qi < nq;
    const float *src = q + (int64_t)(valid ? qi : 0) * dim;
    const float ss = wave_sum_sq(src, dim, lane, valid);
    const float inv = inv_norm_of(ss);  // wave_inv_norm's value
    MetricCoef mc{};
    if constexpr (METRIC) mc = metric_coef(metric, ss);
    float err = 0.f, hh = 0.f;
    for (int c = lane; c < ld; c += 64) {
        const float v = RC_UNIT_ELEM(src, c, dim, inv, valid);
        const f16_t h = Elem<f16_t>::cast(v);
        const float hv = Elem<f16_t>::load(&h, 0);
        const float d = v - hv;
        err = fmaf(d, d, err);
        hh = fmaf(hv, hv, hh);
        if (valid) qn[(int64_t)qi * ld + c] = v;
        qh[(int64_t)qi * ld + c] = h;
    }
    err = wave_sum(err);
    hh = wave_sum(hh);
    if (lane == 0) {
        const float rho = F32F_ROW_NORM_MAX * F32F_ROW_REL + sqrtf((float)ld) * F32F_ROW_ABS;
        const float acc = 6.5e-5f * fmaxf(1.0f, (float)ld * (1.0f / 512.0f));
        const float e = (F32F_ROW_NORM_MAX * i8_resid_bound(err) + i8_resid_bound(hh) * rho + acc) * 1.0001f;
        eps[qi] = e;
        thr[qi] = valid ? -INFINITY : INFINITY;
        if constexpr (METRIC) {
            mcoef[4 * qi + 0] = e;
            mcoef[4 * qi + 1] = mc.alpha;
            mcoef[4 * qi + 2] = mc.beta;
            mcoef[4 * qi + 3] = mc.gamma;
        }
    }
}

struct FilterF32Args {
    FilterArgs a;          // rows: the stored f32 rows; qh: the f16 queries; ld in elements; nqb: blocks of 128·QT queries
    FilterMetric fm;       // METRIC
    const uint32_t *mask;  // MASKED: [ceil(r_end / 32)], over the local rows
    float *dump;           // DUMP: s' of queries [0, dump_nq) x rows [r_begin, r_end), [dump_nq][r_end - r_begin]
    int dump_nq;
};

typedef float f32x8_t __attribute__((ext_vector_type(8)));

template <int NKS, int RT, int QT, bool METRIC, bool MASKED, bool DUMP = false>
__global__ __launch_bounds__(512, 1) void filter_f32_kernel(FilterF32Args fa) {
    static_assert(!(DUMP && (MASKED || METRIC)), "the DUMP form is the cosine filter's s', unmasked");
    using Op = MfmaOp<f16_t>;
    using h8 = Op::v8;
    constexpr int WAVES = 8, QPB = WAVES * 16 * QT, RF = RT / 16;
    constexpr int STEP_BYTES = RT * 128;
    constexpr int NS = QS_NS * 128 / RT;  // ring steps: 128 KB of rows either way
    constexpr int SPS = 2;
    constexpr int PPW = 2 * RF / WAVES;
    constexpr int GF = 2;  // f32 row-fragment slots (8 VGPRs each)
    static_assert((RT == 128 || RT == 64) && (QT == 1 || QT == 2) && NKS % SPS == 0 && (NS - 2 * SPS) * PPW < 64,
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
    const int64_t ldb = a.ld * 4;  // bytes per row
    const int ntiles = (int)(rt1 - rt0);
    const int nsteps = ntiles * NKS;
    const int64_t row0 = a.r_begin + rt0 * RT;  // a multiple of RT (host check)
    const uint8_t *Rg = (const uint8_t *)a.rows + row0 * ldb;

    // this lane's query fragments for the whole K: columns [32 ks + 8 g, + 8) of query q0 + 16 qt + li
    h8 qf[QT][NKS];
    const int q0 = qb * QPB + wave * 16 * QT;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
            qf[qt][ks] = *reinterpret_cast<const h8 *>((const uint16_t *)a.qh + (int64_t)(q0 + qt * 16 + li) * a.ld + ks * 32 + g * 8);
    [[maybe_unused]] float thr[QT];
    [[maybe_unused]] f32x4_t k4[QT];  // METRIC: (eps, alpha, beta, gamma) of the lane's query
    if constexpr (!DUMP) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            thr[qt] = a.thr[q0 + qt * 16 + li];
            if constexpr (METRIC) k4[qt] = *reinterpret_cast<const f32x4_t *>(fa.fm.mcoef + 4 * (q0 + qt * 16 + li));
        }
    }
    // consume the query loads here: the compiler's vmcnt waits for them sit before the K loop
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        if constexpr (!DUMP) {
            asm volatile("" ::"v"(thr[qt]));
            if constexpr (METRIC) asm volatile("" ::"v"(k4[qt]));
        }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) asm volatile("" ::"v"(qf[qt][ks]));
    }

    uint32_t loff[PPW];  // byte offset of this lane's 16 B within the step's rows
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int r = (wave + WAVES * i) * 8 + (lane >> 3);
        loff[i] = (uint32_t)(r * (int)ldb + (((lane & 7) ^ ((r >> 1) & 7)) << 4));
    }
    auto issue = [&](int t) {
        const bool ok = t < nsteps;
        const int tile = t / NKS;
        const int ks = t - tile * NKS;
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
    // this lane's two chunks (2g, 2g + 1, swizzled: the header) of row li of a step's first row group
    const uint8_t *frag_lo = smem + li * 128 + (((2 * g) ^ ((li >> 1) & 7)) << 4);
    const uint8_t *frag_hi = smem + li * 128 + (((2 * g + 1) ^ ((li >> 1) & 7)) << 4);

    f32x4_t acc[RF][QT];
    for (int tile = 0; tile < ntiles; ++tile) {
        const int64_t tile_row = row0 + (int64_t)tile * RT;  // wave-uniform
        [[maybe_unused]] uint32_t mw[RT / 32];  // MASKED: the tile's bitmap words, loaded under its K loop
        if constexpr (MASKED) load_mask_words(fa.mask, tile_row, a.r_end, mw);
#pragma unroll
        for (int rf = 0; rf < RF; ++rf)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) acc[rf][qt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kp = 0; kp < NKS / SPS; ++kp) {
            const int t = tile * NKS + SPS * kp;
            // steps t..t+SPS-1 must have landed; the NS - 2·SPS younger steps (PPW DMAs each, always
            // issued) may be in flight.  What an epilogue issued (loads, atomics) only makes the
            // wait stricter.
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2 * SPS) * PPW) : "memory");
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();  // every wave's DMA of t..t+SPS-1 landed; slots of t-SPS..t-1 are free
            asm volatile("" ::: "memory");
#pragma unroll
            for (int j = NS - SPS; j < NS; ++j) issue(t + j);
            // The sync group's SPS·RF row fragments f = (k-step kl, row group rf), GF f32 slots, rolling:
            // fragment f is converted, its QT MFMAs issue, and fragment f + GF is read into its slot,
            // so the LDS latency runs under the MFMAs between.
            constexpr int NF = SPS * RF;
            // the ring slot of step t + kl: a tile is a whole number of ring turns where NKS % NS == 0, and
            // the slot is then a constant of the unrolled loop (an immediate offset of the read)
            const int s0 = NKS % NS == 0 ? SPS * kp : t;
            auto read_frag = [&](int f) {
                const int kl = f / RF, rf = f % RF;
                const int so = ((s0 + kl) % NS) * STEP_BYTES + 16 * rf * 128;
                const f32x4_t lo = *reinterpret_cast<const f32x4_t *>(frag_lo + so);
                const f32x4_t hi = *reinterpret_cast<const f32x4_t *>(frag_hi + so);
                return (f32x8_t)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            };
            f32x8_t cur[GF];
#pragma unroll
            for (int f = 0; f < GF; ++f) cur[f] = read_frag(f);
            __builtin_amdgcn_sched_barrier(0);  // the first GF fragments' reads go out together, ahead of the pattern
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const int ks = SPS * kp + f / RF, rf = f % RF;
                const h8 x16 = __builtin_convertvector(cur[f % GF], h8);  // 4 x v_cvt_pk_f16_f32 (RNE): the header's x̃
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) acc[rf][qt] = Op::mma(x16, qf[qt][ks], acc[rf][qt]);
                if (f + GF < NF) cur[f % GF] = read_frag(f + GF);
                __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, QT, 0);
                if (f + GF < NF) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            }
            // pin the accumulators here: the step issue's branches split the basic block, and the
            // compiler otherwise sinks this sync group's MFMAs into the next one's block
#pragma unroll
            for (int rf = 0; rf < RF; ++rf)
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) asm volatile("" : "+v"(acc[rf][qt]));
        }
        // rows in 32 bits from here (a local row is below the capacity, < 2^32): the tile's first row
        // of this lane, and how many rows from it are inside the range
        const uint32_t rbase = (uint32_t)tile_row + 4u * (uint32_t)g;
        const int64_t left64 = a.r_end - tile_row - 4 * g;
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
        // ---- epilogue of the tile: candidates s' >= thr[q] (METRIC: u >= thr[q])
        if constexpr (MASKED) {  // no eligible row in the tile: no epilogue (wave-uniform)
            uint32_t any = 0u;
#pragma unroll
            for (int i = 0; i < RT / 32; ++i) any |= mw[i];
            if (any == 0u) continue;
        }
        if constexpr (METRIC) {  // in place: the accumulators become u (the metric epilogue's comment in filter_mfma.h)
            __builtin_amdgcn_sched_barrier(0);  // nothing of this moves up among the tile's last MFMAs, where the staging is live
            const float *tn = fa.fm.norms + tile_row;
            const int left_t = (int)min<int64_t>(a.r_end - tile_row, (int64_t)RT);  // >= 1: the tile has a row in range
#pragma unroll
            for (int rf = 0; rf < RF; ++rf) {
                const f32x4_t nv = load_norms4(tn, 4 * g + rf * 16, left_t);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[rf][qt][j] = metric_upper(k4[qt], acc[rf][qt][j], nv[j]);
                if (rf % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // at most two norm loads (8 registers) in flight
            }
        }
        if constexpr (MASKED) {
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

// ------------------------------------------------------------------ host ---
bool f32_filter_supported(int64_t ld) { return ld == 128 || ld == 256 || ld == 512 || ld == 768; }

void prepare_queries_f32(const BatchPlan &p, const BatchWs &ws, int nq_pad, hipStream_t s) {
    if (p.metric != RC_METRIC_COSINE)
        hipLaunchKernelGGL(prepare_queries_f32_kernel<true>, dim3(nq_pad), dim3(64), 0, s, p.queries, p.nq, p.dim, p.ld, p.metric, ws.qn.get(),
                           (f16_t *)ws.qh.get(), ws.eps.get(), ws.thr.get(), ws.mcoef.get());
    else
        hipLaunchKernelGGL(prepare_queries_f32_kernel<false>, dim3(nq_pad), dim3(64), 0, s, p.queries, p.nq, p.dim, p.ld, p.metric, ws.qn.get(),
                           (f16_t *)ws.qh.get(), ws.eps.get(), ws.thr.get(), ws.mcoef.get());
    RC_LAUNCH_CHECK();
}

// One width's kernels: the form by the plan's metric and mask, or (dump != null) the DUMP form.
template <int NKS, int RT, int QT>
void launch_filter_f32_shape(const BatchPlan &p, const BatchWs &ws, int nq_pad, int64_t c0, int64_t c1, int64_t nchunk, float *dump,
                             hipStream_t s) {
    const int nqb = nq_pad / (128 * QT);
    RC_REQUIRE(c0 % RT == 0, RC_ERR_INVALID, "internal: float32 filter range not tile-aligned");
    const bool metric = p.metric != RC_METRIC_COSINE, masked = p.mask_filter;
    const FilterF32Args fa{FilterArgs{p.rows, ws.qh.get(), p.ld, NKS, c0, c1, tiles_per_chunk(c0, c1, RT, nchunk), nqb, ws.thr.get(), ws.cnt.get(), ws.cand.get(), ws.cap},
                           FilterMetric{p.norms, ws.mcoef.get()}, p.mask, dump, p.nq};
    const dim3 gr((unsigned)(nchunk * nqb)), bl(512);
    if (dump != nullptr) hipLaunchKernelGGL((filter_f32_kernel<NKS, RT, QT, false, false, true>), gr, bl, 0, s, fa);
    else if (metric && masked) hipLaunchKernelGGL((filter_f32_kernel<NKS, RT, QT, true, true>), gr, bl, 0, s, fa);
    else if (metric) hipLaunchKernelGGL((filter_f32_kernel<NKS, RT, QT, true, false>), gr, bl, 0, s, fa);
    else if (masked) hipLaunchKernelGGL((filter_f32_kernel<NKS, RT, QT, false, true>), gr, bl, 0, s, fa);
    else hipLaunchKernelGGL((filter_f32_kernel<NKS, RT, QT, false, false>), gr, bl, 0, s, fa);
}

void launch_filter_f32(const BatchPlan &p, const BatchWs &ws, int nq_pad, int64_t c0, int64_t c1, int64_t nchunk, float *dump,
                       hipStream_t s) {
    switch (p.ld) {  // the header's shapes
    case 128: return launch_filter_f32_shape<4, 128, 2>(p, ws, nq_pad, c0, c1, nchunk, dump, s);
    case 256: return launch_filter_f32_shape<8, 64, 2>(p, ws, nq_pad, c0, c1, nchunk, dump, s);
    case 512: return launch_filter_f32_shape<16, 64, 2>(p, ws, nq_pad, c0, c1, nchunk, dump, s);
    case 768: return launch_filter_f32_shape<24, 64, 1>(p, ws, nq_pad, c0, c1, nchunk, dump, s);
    default: throw Error(RC_ERR_UNSUPPORTED, "the float32 filter needs a row width (dim rounded up to 128) of 128, 256, 512 or 768");
    }
}

// rc_index_filter_scores: the float32 filter's own s' (the DUMP form) and eps, under the cosine
// preparation whatever the index's metric (eps is the same number under a metric: mcoef[q][0])
void filter_scores_f32(const BatchPlan &p, BatchWs &ws, int64_t row0, int64_t n, float *out_scores, float *out_eps, hipStream_t s) {
    RC_REQUIRE(f32_filter_supported(p.ld), RC_ERR_UNSUPPORTED, "the float32 filter needs ld 128, 256, 512 or 768");
    const int nq_pad = (p.nq + SB_TILE - 1) / SB_TILE * SB_TILE;
    prepare_queries_f32(p, ws, nq_pad, s);
    launch_filter_f32(p, ws, nq_pad, row0, row0 + n, 8, out_scores, s);
    RC_LAUNCH_CHECK();
    RC_HIP(hipMemcpyAsync(out_eps, ws.eps.get(), (size_t)p.nq * sizeof(float), hipMemcpyDeviceToDevice, s));
}

}  // namespace rc
