// qkv_attention.h — the QKV projection fused into self-attention for the model's real shape
// (197 tokens, hidden 768, 12 heads of 64, LayerNorm fold on): one workgroup per (image, head)
// computes that head's Q, K and V (208 x 192, K = 768) from the image's rows of the bf16
// residual stream straight into LDS and runs attention from there.  What it removes: the qkv
// tensor's round trip through HBM (gemm_pp_kernel<EPI_BF16_LN> writes 3 x 768 bf16 per token,
// attention_v2_kernel reads them straight back).
//
// Same bits as the two kernels it replaces: every output element is the same chain of
// mfma_f32_16x16x32_bf16 (weight fragment first, K blocks ascending, lane group g holding k =
// 32 kt + 8 g ..) as pp_kloop / gemm_w2_kernel, the LN-fold consumer epilogue is pp_epilogue's
// (ln_apply4, the one function both call) rounded with pack_bf16x2, and the attention phase is
// att_scores<197> / att_pv_store on K and V in the LDS layouts attention_v2_kernel stages.
//
// GEMM phase (gemm_w2_kernel's loop): 4 waves, wave w owns all 13 row blocks x output columns
// [48 w, 48 w + 48) of [Q | K | V] = acc[13][3], 156 accumulator VGPRs — splitting the columns
// keeps the 13th row block balanced over the waves.  Operands by LDS-DMA into a 3-slot ring of
// BK = 32 steps: slot = A 208 rows (rows 197..207 clamped to 196, as attention pads its keys) +
// W 192 rows (the head's three 64-row slices of W') of 64 B, chunk c of row r stored at
// c ^ (((r >> 3) & 1) << 1).  25 pieces of 1 KB per slot: wave 0 issues 7, the others 6.
// Epilogue: the ring is dead after the loop's last reads, and Q, K, V (3 x 208 x 128 B =
// 79 872 B) take its place — Q and K rows with the chunk swizzle (row >> 1) & 7, V with
// ((row >> 1) & 3) << 1.  The rows' (rstd, -rstd·mu) sit behind them.  81 536 B in all: two
// workgroups per CU (160 KB), one in its attention phase beside the other's K loop.
//
// Block order: blockIdx b runs on XCD b % 8.  XCD x takes the heads 3 (x & 3) .. + 2 for the
// images of parity x >> 2, three heads of one image on consecutive blocks: an XCD's L2 keeps
// its three heads' W slices (885 KB) for the whole launch and streams each A panel once for
// the three blocks that read it at the same time.
//
// Measured against this form at batch 256 (DESIGN.md § QKV + attention fusion; bit-identical
// all): image-major block ids and six heads per XCD within 1 %; the A rows staged nontemporal
// +27 % per launch; one 8-wave workgroup per (image, pair of heads) sharing the A stage (26 %
// fewer staged bytes, one workgroup per CU) +1 %, its ring 4 deep +3 %; s_setprio(1) around the
// MFMAs +5 %.  Neither the staged bytes nor the L2 locality bound the K loop.
//
// The wave schedule inside a K-step did ("the wave schedule", profiles/qkv_sched/): as
// hipcc laid the step out, a wave issued its 6-7 DMA pieces, then 11 fragment reads, waited for
// all of them and only then started its 39 MFMAs, and the epilogue was a chain of exposed LDS and
// L2 round trips.  The product form (QA_SCHED) reads the fragments first, starts row block mi's
// MFMAs once its own fragment has landed, spreads the DMA pieces among the MFMAs and loads the
// epilogue's operands before the barrier that frees the ring: 230 -> 214 us per launch, same bits.
// Diagnostic builds keep the earlier forms as variants beside it for the phase stamps.
#pragma once

#include <type_traits>

#include "gemm.h"

namespace rc {

struct QkvAttnArgs {
    const uint16_t *x;      // [n · 197][768] bf16 residual stream
    const uint16_t *w;      // [3 · 768][768] bf16 W' = W_qkv · diag(γ)
    const float *bias;      // [3 · 768] b' = b + W·β
    const float *ln_c;      // [3 · 768] c = Σ_k W'
    const float *ln_stats;  // [n · 197][LN_PARTS][2]
    uint16_t *out;          // [n · 197][768] attention output
    int n;                  // images
    float ln_eps, scale_log2e;
};

constexpr int QA_TOK = 197, QA_H = 768, QA_HEADS = 12, QA_HD = 64, QA_WAVES = 4;
constexpr int QA_BK = 32, QA_NSLOT = 3, QA_NK = QA_H / QA_BK;
constexpr int QA_WROWS = 3 * QA_HD;                                   // 192 weight rows of a head
constexpr int QA_A_BYTES = ATT2_ROWS * QA_BK * 2;                     // 13 312
constexpr int QA_SLOT = QA_A_BYTES + QA_WROWS * QA_BK * 2;            // 25 600
constexpr int QA_A_PIECES = ATT2_TILES, QA_PIECES = QA_SLOT / 1024;   // 13 A + 12 W
constexpr int QA_PPW = (QA_PIECES + 3) / 4, QA_PPW_LO = QA_PIECES / 4;
constexpr int QA_MAT = ATT2_ROWS * QA_HD * 2;                         // one of Q / K / V: 26 624
constexpr int QA_LN_OFF = 3 * QA_MAT, QA_LDS = QA_LN_OFF + ATT2_ROWS * 8;
static_assert(QA_NSLOT * QA_SLOT <= QA_LN_OFF, "Q, K and V alias the ring; the row scales lie behind both");
static_assert(2 * QA_LDS <= 160 * 1024, "two workgroups per CU");

// grid for n images: 8 XCDs x 3 heads x ceil(n / 2) images of one parity
inline int qkv_attention_grid(int n) { return 8 * 3 * ((n + 1) / 2); }

// Schedule variants (bits of SCHED; every one leaves each output bit alone):
//   QA_S_EPI    the epilogue's loads (the wave's 13 row scales, bias and c of its three column
//               blocks) issued after the K loop's last MFMAs, before the barrier that frees the ring
//   QA_S_KSTEP  a K-step reads its fragments first (inline-asm ds_reads behind counted lgkmcnt waits:
//               row block mi's MFMAs wait for its own fragment only) and issues its DMA pieces
//               among the MFMAs, one behind every second row block
// STAMP (diagnostic builds): s_memrealtime at block entry, K loop start / end, epilogue end and each
// wave's end into g_rc_stamps[QA_STAMP_BASE + 16 · block ..] (tools/qkv_sched_ab.py) — behind the
// region the tiled GEMMs of the same step stamp (64 per workgroup, gemm.h).
constexpr int QA_S_EPI = 1, QA_S_KSTEP = 2;
constexpr int64_t QA_STAMP_BASE = 1 << 20;

// Inline-asm LDS fragment reads that hipcc does not count, and the counted waits tied to their
// registers (gemm_skinny.h's form).  qa_ds_reread overwrites a fragment in place ("+v": it stays
// behind the MFMAs that read the register), qa_pin keeps a register's readers above this point.
template <int OFF>
__device__ __forceinline__ void qa_ds_read(bf16x8 &x, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(x) : "v"(addr), "n"(OFF));
}
template <int OFF>
__device__ __forceinline__ void qa_ds_reread(bf16x8 &x, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "+v"(x) : "v"(addr), "n"(OFF));
}
__device__ __forceinline__ void qa_pin(bf16x8 &x) { asm volatile("" : "+v"(x)); }
template <int N>
__device__ __forceinline__ void qa_wait_lgkm(bf16x8 &x) {
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(x) : "n"(N));
}
template <int N>
__device__ __forceinline__ void qa_wait_lgkm(bf16x8 &x, bf16x8 &y, bf16x8 &z, bf16x8 &w) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(x), "+v"(y), "+v"(z), "+v"(w) : "n"(N));
}
// f(integral_constant<int, I>) for I = I0 .. N - 1: indices that inline asm takes as immediates
template <int I, int N, class F>
__device__ __forceinline__ void qa_static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        qa_static_for<I + 1, N>(f);
    }
}

template <int SCHED, bool STAMP>
__device__ __forceinline__ void qkv_attention_body(const QkvAttnArgs &a) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[QA_LDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;

    const int xcd = blockIdx.x & 7, bj = blockIdx.x >> 3;
    const int h = 3 * (xcd & 3) + bj % 3, img = 2 * (bj / 3) + (xcd >> 2);
    if (img >= a.n) return;  // odd n: the odd-parity XCDs have one image fewer
    const int64_t row0 = (int64_t)img * QA_TOK;

    // piece p (1 KB = 16 rows x 64 B): 0..12 A rows 16 p .., then local W rows 16 (p - 13) ..
    // (local row c = 64 · {q, k, v} + d -> row {0, 768, 1536} + 64 h + d of W').  Lane l writes
    // LDS bytes [16 l, 16 l + 16) of the piece: row l >> 2, stored chunk l & 3, which holds
    // source chunk (l & 3) ^ (((l >> 5) & 1) << 1).
    const int prow = lane >> 2, pchunk = (lane & 3) ^ (((lane >> 5) & 1) << 1);
    const uint16_t *srcp[QA_PPW];
#pragma unroll
    for (int i = 0; i < QA_PPW; ++i) {
        const int piece = min(wave + 4 * i, QA_PIECES - 1);  // wave-uniform
        if (piece < QA_A_PIECES) {
            srcp[i] = a.x + (row0 + min(piece * 16 + prow, QA_TOK - 1)) * QA_H;
        } else {
            const int c = (piece - QA_A_PIECES) * 16 + prow;
            srcp[i] = a.w + (int64_t)((c >> 6) * QA_H + h * QA_HD + (c & 63)) * QA_H;
        }
        srcp[i] += pchunk * 8;
    }
    auto stage_piece = [&](int slot, int k0, int i) __attribute__((always_inline)) {
        const int piece = wave + 4 * i;
        if (i >= QA_PPW_LO && piece >= QA_PIECES) return;  // the 7th piece: wave 0 only
        __builtin_amdgcn_global_load_lds((const void *)(srcp[i] + k0),
                                         (lds_void_t *)(smem + slot * QA_SLOT + piece * 1024), 16, 0, 0);
    };
    auto stage = [&](int slot, int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < QA_PPW; ++i) stage_piece(slot, k0, i);
    };
    auto bar = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    const int fchunk = (g ^ (((li >> 3) & 1) << 1)) << 4;

    f32x4 acc[ATT2_TILES][3];
#pragma unroll
    for (int i = 0; i < ATT2_TILES; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // diagnostic builds: stamp `idx` of this block, written by lane 0 of wave 0 or of every wave
    auto stamp = [&](int idx, bool every_wave) __attribute__((always_inline)) {
#if defined(RC_GEMM_ABLATION)
        if constexpr (STAMP)
            if (g_rc_stamps != nullptr && lane == 0 && (every_wave || wave == 0))
                g_rc_stamps[QA_STAMP_BASE + (int64_t)blockIdx.x * 16 + idx] = RC_NOW();
#endif
    };
    stamp(0, false);

    stage(0, 0);
    stage(1, QA_BK);
    // the rows' LayerNorm scales, under the first DMA (pad rows: row 196's, as their A rows)
    if (tid < ATT2_ROWS)
        *reinterpret_cast<float2 *>(smem + QA_LN_OFF + tid * 8) =
            ln_row_scale(a.ln_stats + (row0 + min(tid, QA_TOK - 1)) * LN_STRIDE, a.ln_eps);

    // W and the first QA_AF row fragments are read first, then each later row fragment behind the
    // MFMAs of an earlier row block (whose registers it takes: 13 fragments live would spill)
    constexpr int QA_AF = 8;
    // QA_S_KSTEP counts its own ds_reads in lgkmcnt: no scalar load may be in flight beside them
    if constexpr ((SCHED & QA_S_KSTEP) != 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const uint32_t frag0 = (uint32_t)(uintptr_t)smem + li * 64 + fchunk;  // QA_S_KSTEP: the lane's fragment in row block 0
    stamp(1, false);

    for (int kt = 0; kt < QA_NK; ++kt) {
        // raw s_barrier behind a counted wait: the next slot's pieces of this wave may still fly
        if (kt + 1 < QA_NK) {
            if (wave < QA_PIECES % 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(QA_PPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(QA_PPW_LO) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        bar();
        if constexpr ((SCHED & QA_S_KSTEP) == 0) {
            if (kt + 2 < QA_NK) stage((kt + 2) % QA_NSLOT, (kt + 2) * QA_BK);
            const uint8_t *As = smem + (kt % QA_NSLOT) * QA_SLOT;
            const uint8_t *Ws = As + QA_A_BYTES;
            bf16x8 wf[3], af[ATT2_TILES];
#pragma unroll
            for (int ni = 0; ni < 3; ++ni)
                wf[ni] = *reinterpret_cast<const bf16x8 *>(Ws + (wave * 48 + ni * 16 + li) * 64 + fchunk);
#pragma unroll
            for (int mi = 0; mi < ATT2_TILES; ++mi)
                af[mi] = *reinterpret_cast<const bf16x8 *>(As + (mi * 16 + li) * 64 + fchunk);
#pragma unroll
            for (int mi = 0; mi < ATT2_TILES; ++mi)
#pragma unroll
                for (int ni = 0; ni < 3; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ni], af[mi], acc[mi][ni], 0, 0, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 3 + QA_AF, 0);
#pragma unroll
            for (int i = 0; i < ATT2_TILES - QA_AF; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 3 * QA_AF, 0);
        } else {
            // The order of these volatile statements is the schedule.  The fragment reads go first;
            // row block mi's MFMAs sit behind a counted wait tied to their fragment (the reads retire
            // in order: at most 7 younger ones are in flight), and the refill of slot (kt + 2) % 3 —
            // last read in step kt - 1, before this step's barrier — is spread among them, piece j
            // behind row block 2 j + 1 (the 7th behind the last).  Every read has retired at the last
            // row block's lgkmcnt(0), before the next barrier; the pieces keep their order, so the
            // vmcnt above still leaves exactly the newest group in flight.
            const bool fill = kt + 2 < QA_NK;
            const int s2 = (kt + 2) % QA_NSLOT, k2 = (kt + 2) * QA_BK;
            const uint32_t pa = frag0 + (kt % QA_NSLOT) * QA_SLOT, pw = pa + QA_A_BYTES + wave * (48 * 64);
            bf16x8 wf[3], af[QA_AF];
            qa_static_for<0, 3>([&](auto ic) {
                constexpr int ni = decltype(ic)::value;
                qa_ds_read<ni * 1024>(wf[ni], pw);
            });
            qa_static_for<0, QA_AF>([&](auto ic) {
                constexpr int mi = decltype(ic)::value;
                qa_ds_read<mi * 1024>(af[mi], pa);
            });
            qa_static_for<0, ATT2_TILES>([&](auto ic) {
                constexpr int mi = decltype(ic)::value, r = mi % QA_AF;
                constexpr int later = ATT2_TILES - QA_AF;  // fragments read behind the MFMAs
                // in flight behind fragment mi: the rest of the first QA_AF and the later ones issued so far
                constexpr int younger = mi < QA_AF ? (QA_AF - 1 - mi) + (mi < later ? mi : later) : ATT2_TILES - 1 - mi;
                if constexpr (mi == 0) {
                    qa_wait_lgkm<younger>(wf[0], wf[1], wf[2], af[0]);
                } else {
                    qa_wait_lgkm<younger>(af[r]);
                }
#pragma unroll
                for (int ni = 0; ni < 3; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ni], af[r], acc[mi][ni], 0, 0, 0);
                if constexpr (mi + QA_AF < ATT2_TILES) {  // "+v": behind the MFMAs that read the register
                    qa_ds_reread<(mi + QA_AF) * 1024>(af[r], pa);
                } else {
                    qa_pin(af[r]);
                }
                if constexpr (mi % 2 == 1 && mi / 2 < QA_PPW - 1) {
                    if (fill) stage_piece(s2, k2, mi / 2);
                } else if constexpr (mi == ATT2_TILES - 1) {
                    if (fill) stage_piece(s2, k2, QA_PPW - 1);
                }
            });
        }
    }
    stamp(2, false);
    // QA_S_EPI: the epilogue's loads here, under the barrier and under each other (the fragment
    // registers are dead): the wave's 13 row scales, once, and bias and c of its three column blocks
    constexpr bool EPI = (SCHED & QA_S_EPI) != 0;
    float2 rs[EPI ? ATT2_TILES : 1];
    float4 b4s[EPI ? 3 : 1], c4s[EPI ? 3 : 1];
    if constexpr (EPI) {
#pragma unroll
        for (int ni = 0; ni < 3; ++ni) {
            const int c0 = wave * 48 + ni * 16, gcol = (c0 >> 6) * QA_H + h * QA_HD + (c0 & 63) + 4 * g;
            b4s[ni] = *reinterpret_cast<const float4 *>(a.bias + gcol);
            c4s[ni] = *reinterpret_cast<const float4 *>(a.ln_c + gcol);
        }
#pragma unroll
        for (int mi = 0; mi < ATT2_TILES; ++mi)
            rs[mi] = *reinterpret_cast<const float2 *>(smem + QA_LN_OFF + (mi * 16 + li) * 8);
    }
    bar();  // every wave's last fragment reads are done: Q, K, V may overwrite the ring

    // epilogue: acc[mi][ni][j] = [Q | K | V][mi·16 + li][48 wave + 16 ni + 4 g + j]
    // (one 16-column block at a time: its bias and c in registers beside the accumulators)
#pragma unroll
    for (int ni = 0; ni < 3; ++ni) {
        const int c0 = wave * 48 + ni * 16, mat = c0 >> 6, d = (c0 & 63) + 4 * g;
        const int gcol = mat * QA_H + h * QA_HD + d;
        float4 b4, c4;
        if constexpr (EPI) {
            b4 = b4s[ni];
            c4 = c4s[ni];
        } else {
            b4 = *reinterpret_cast<const float4 *>(a.bias + gcol);
            c4 = *reinterpret_cast<const float4 *>(a.ln_c + gcol);
        }
        uint8_t *mbase = smem + mat * QA_MAT + (d & 7) * 2;
#pragma unroll
        for (int mi = 0; mi < ATT2_TILES; ++mi) {
            const int row = mi * 16 + li;
            float2 r;
            if constexpr (EPI) r = rs[mi];
            else r = *reinterpret_cast<const float2 *>(smem + QA_LN_OFF + row * 8);
            const float4 v = ln_apply4(r, acc[mi][ni], c4, b4);
            const int swz = mat == 2 ? ((row >> 1) & 3) << 1 : (row >> 1) & 7;
            *reinterpret_cast<uint2 *>(mbase + row * 128 + (((d >> 3) ^ swz) << 4)) = pack_bf16x4(v);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    stamp(3, false);

    // attention: query tiles wave, wave + 4, ..; Q fragments from LDS in load_q's layout
    const uint8_t *Qs = smem, *Ks = smem + QA_MAT, *Vs = smem + 2 * QA_MAT;
    uint16_t *obase = a.out + row0 * QA_H + h * QA_HD;
    for (int qt = wave; qt < ATT2_TILES; qt += 4) {
        const int r = qt * 16 + li;
        bf16x8 qf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
            qf[s] = *reinterpret_cast<const bf16x8 *>(Qs + r * 128 + (((s * 4 + g) ^ ((r >> 1) & 7)) << 4));
        f32x4 st[ATT2_TILES];
        float sum = 0.f;
        att_scores<QA_TOK>(Ks, qf, QA_TOK, a.scale_log2e, st, sum);
        att_pv_store(Vs, st, sum, qt, QA_TOK, obase, QA_H);
    }
    stamp(4 + wave, true);
#if defined(RC_GEMM_ABLATION)
    if constexpr (STAMP)  // XCC_ID | HW_ID: which CU ran the block
        if (g_rc_stamps != nullptr && tid == 0)
            g_rc_stamps[QA_STAMP_BASE + (int64_t)blockIdx.x * 16 + 8] = (uint64_t)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |
                                                       ((uint64_t)__builtin_amdgcn_s_getreg(20 | (3 << 11)) << 32);
#endif
}

// The product's schedule.  Measured per launch at batch 256, four interleaved rounds in one process
// (profiles/qkv_sched/variants_sched.jsonl): neither 230.0, QA_S_EPI alone 232.4 (its registers
// spill beside the compiler-scheduled K-step), QA_S_KSTEP alone 220.6, both 213.6 us.
constexpr int QA_SCHED = QA_S_EPI | QA_S_KSTEP;

__global__ __launch_bounds__(64 * QA_WAVES, 2) void qkv_attention_kernel(QkvAttnArgs a) {
    qkv_attention_body<QA_SCHED, false>(a);
}

#if defined(RC_GEMM_ABLATION)
// diagnostic builds: every schedule variant, and the phase stamps, for in-process A/B (rc_diag_set_qkv_sched)
template <int SCHED, bool STAMP>
__global__ __launch_bounds__(64 * QA_WAVES, 2) void qkv_attention_diag_kernel(QkvAttnArgs a) {
    qkv_attention_body<SCHED, STAMP>(a);
}
// v = schedule bits (0 .. 3) + 8 for the stamps
inline void launch_qkv_attention_diag(int v, const QkvAttnArgs &q, int n, hipStream_t s) {
    const dim3 grid(qkv_attention_grid(n)), block(64 * QA_WAVES);
    switch (v) {
#define QA_DIAG_CASE(V)                                                                              \
    case V: hipLaunchKernelGGL((qkv_attention_diag_kernel<V, false>), grid, block, 0, s, q); break; \
    case V + 8: hipLaunchKernelGGL((qkv_attention_diag_kernel<V, true>), grid, block, 0, s, q); break;
        QA_DIAG_CASE(0)
        QA_DIAG_CASE(1)
        QA_DIAG_CASE(2)
        QA_DIAG_CASE(3)
#undef QA_DIAG_CASE
        default: throw Error(RC_ERR_INVALID, "QKV schedule variant: 0 .. 3 (+ 8: stamps)");
    }
}
#endif

}  // namespace rc
