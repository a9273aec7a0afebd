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
#pragma once

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

__global__ __launch_bounds__(64 * QA_WAVES, 2) void qkv_attention_kernel(QkvAttnArgs a) {
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
    auto stage = [&](int slot, int k0) {
        uint8_t *base = smem + slot * QA_SLOT;
#pragma unroll
        for (int i = 0; i < QA_PPW; ++i) {
            const int piece = wave + 4 * i;
            if (i >= QA_PPW_LO && piece >= QA_PIECES) continue;  // the 7th piece: wave 0 only
            __builtin_amdgcn_global_load_lds((const void *)(srcp[i] + k0), (lds_void_t *)(base + piece * 1024), 16, 0, 0);
        }
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

    stage(0, 0);
    stage(1, QA_BK);
    // the rows' LayerNorm scales, under the first DMA (pad rows: row 196's, as their A rows)
    if (tid < ATT2_ROWS)
        *reinterpret_cast<float2 *>(smem + QA_LN_OFF + tid * 8) =
            ln_row_scale(a.ln_stats + (row0 + min(tid, QA_TOK - 1)) * LN_STRIDE, a.ln_eps);

    for (int kt = 0; kt < QA_NK; ++kt) {
        // raw s_barrier behind a counted wait: the next slot's pieces of this wave may still fly
        if (kt + 1 < QA_NK) {
            if (wave < QA_PIECES % 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(QA_PPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(QA_PPW_LO) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        bar();
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
        // W and the first QA_AF row fragments first, then each later row fragment behind the MFMAs
        // of an earlier row block (whose registers it takes: 13 fragments live would spill)
        constexpr int QA_AF = 8;
        __builtin_amdgcn_sched_group_barrier(0x100, 3 + QA_AF, 0);
#pragma unroll
        for (int i = 0; i < ATT2_TILES - QA_AF; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 3 * QA_AF, 0);
    }
    bar();  // every wave's last fragment reads are done: Q, K, V may overwrite the ring

    // epilogue: acc[mi][ni][j] = [Q | K | V][mi·16 + li][48 wave + 16 ni + 4 g + j]
    // (one 16-column block at a time: its bias and c in registers beside the accumulators)
#pragma unroll
    for (int ni = 0; ni < 3; ++ni) {
        const int c0 = wave * 48 + ni * 16, mat = c0 >> 6, d = (c0 & 63) + 4 * g;
        const int gcol = mat * QA_H + h * QA_HD + d;
        const float4 b4 = *reinterpret_cast<const float4 *>(a.bias + gcol);
        const float4 c4 = *reinterpret_cast<const float4 *>(a.ln_c + gcol);
        uint8_t *mbase = smem + mat * QA_MAT + (d & 7) * 2;
#pragma unroll
        for (int mi = 0; mi < ATT2_TILES; ++mi) {
            const int row = mi * 16 + li;
            const float2 r = *reinterpret_cast<const float2 *>(smem + QA_LN_OFF + row * 8);
            const float4 v = ln_apply4(r, acc[mi][ni], c4, b4);
            const int swz = mat == 2 ? ((row >> 1) & 3) << 1 : (row >> 1) & 7;
            *reinterpret_cast<uint2 *>(mbase + row * 128 + (((d >> 3) ^ swz) << 4)) = pack_bf16x4(v);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();

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
}

}  // namespace rc
