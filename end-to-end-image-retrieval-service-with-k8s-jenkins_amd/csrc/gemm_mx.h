// gemm_mx.h — the MXFP8 MLP (rc_model_set_mlp_dtype(1)): the OCP MX format, its quantise
// kernel, and fc2 as a block-scaled fp8 GEMM.  (fc1's MXFP8 epilogue lives with the kernel
// that runs it: pp_epilogue in gemm.h.)
//
// Format: blocks of 32 consecutive elements along K share one E8M0 scale byte.  With a = max|x|
// of the block, e = floor(log2 a) − 8, one more if a > 448·2^e (so a·2^−e <= 448, the largest
// e4m3 value: nothing saturates), clamped to [−127, 127]; a == 0 gives e = −127 and zero bytes.
// The scale byte is e + 127, an element the e4m3fn value nearest x·2^−e (ties to even).  Rows are
// row-major: bytes [rows][K], scales [rows][K / 32].
//
// fc2: C[M][N] += A[M][K]·W[N][K]ᵀ + bias on v_mfma_scale_f32_16x16x128_f8f6f4 (K = 128 per
// instruction, both operands e4m3, per-lane E8M0 scales).  Operand layout, as measured on the
// device with one-hot chunks and one-hot scales: lane (g = lane >> 4, li = lane & 15) holds row
// li's K bytes [16 g, 16 g + 16) in its first four registers and [64 + 16 g, 64 + 16 g + 16) in
// its last four, while byte 0 of its scale register scales K block g, bytes [32 g, 32 g + 32) —
// held by lane groups 2 (g & 1) and 2 (g & 1) + 1 of the same row, in the half g >> 1.  So a lane's
// 32 bytes are halves of two MX blocks, and the scale it supplies is not the scale of its own
// bytes.  (The float8 search filter, all scales equal, is indifferent to this.)
// Tile 256 x 256 x 128, 512 threads = 8 waves as 2 (M) x 4 (N), each wave 128 x 64 outputs =
// acc[8][4] (the two-workgroup kernel's per-wave layout, whose epilogue it calls).  A K-step is
// 128 B of each of the 512 rows: 64 KB, the bf16 ping-pong kernel's bytes per step for twice the
// K, fed by half as many steps.  Ring: 2 slots x (A 32 KB + W 32 KB + 2 KB of scales), rows of
// 128 B with the 16-B chunk XOR-swizzled by (row >> 1) & 7 (a fragment is two conflict-free
// ds_read_b128).  The scales ride the same LDS-DMA: per K-step a row's four scale bytes are one
// aligned dword, 512 dwords per step, one 4-B-per-lane DMA per wave; a lane reads its row's
// dword and shifts its block's byte (g = lane >> 4) down — no separate scale pass, no re-layout.
// One barrier per K-step: wait for this slot, barrier, issue the next slot's DMA, then 12
// fragments and 32 MFMAs per wave (the slot's DMA lands under them).
// Row tiles are the plain 256-row ones, not image-aligned: at parts = 2 the bf16 fc2 measured
// slower on image-aligned tiles (gemm_pick's comment), and A rows past M are clamped here, so
// the kernel needs no padded A.
#pragma once

#include "gemm.h"

namespace rc {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// (mx_scale_byte / mx_inv_scale / mx_pack4, the rule on the f32 bits: gemm.h)

// Quantise src [R][K] (f32 or bf16) to MXFP8.  Eight lanes per block, four elements each: the
// block maximum by three xor shuffles, 4-B stores (a wave writes 256 contiguous bytes).
template <typename T>
__global__ __launch_bounds__(256) void mxfp8_quantize_kernel(const T *src, int64_t nblocks, uint8_t *q, uint8_t *scales) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t blk = t >> 3;
    const bool ok = blk < nblocks;  // whole groups of 8 lanes, so the shuffles stay inside live lanes
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (ok) {
        if constexpr (sizeof(T) == 4) {
            const float4 x = *reinterpret_cast<const float4 *>(src + 4 * t);
            v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
        } else {
            const float4 x = bf16x4_f32(*reinterpret_cast<const uint2 *>(src + 4 * t));
            v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
        }
    }
    float am = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) am = fmaxf(am, __shfl_xor(am, d));
    const uint32_t sb = mx_scale_byte(am);
    const float inv = mx_inv_scale(sb);
    if (ok) {
        *reinterpret_cast<uint32_t *>(q + 4 * t) = mx_pack4(v[0] * inv, v[1] * inv, v[2] * inv, v[3] * inv);
        if ((t & 7) == 0) scales[blk] = (uint8_t)sb;
    }
}

inline void launch_mxfp8_quantize(const void *src, bool bf16, int64_t rows, int K, uint8_t *q, uint8_t *scales, hipStream_t s) {
    const int64_t nblocks = rows * (K / 32);
    const dim3 gr((unsigned)((nblocks * 8 + 255) / 256));
    if (bf16) hipLaunchKernelGGL(mxfp8_quantize_kernel<uint16_t>, gr, dim3(256), 0, s, (const uint16_t *)src, nblocks, q, scales);
    else hipLaunchKernelGGL(mxfp8_quantize_kernel<float>, gr, dim3(256), 0, s, (const float *)src, nblocks, q, scales);
    RC_LAUNCH_CHECK();
}

struct MxGemmArgs {
    const uint8_t *A8, *As;  // [M][K] e4m3, [M][K / 32] E8M0
    const uint8_t *W8, *Ws;  // [N][K], [N][K / 32]
    GemmArgs g;              // bias, M, N, K and the residual epilogue's arrays (A / W unused)
};

constexpr int MX_BM = 256, MX_BN = 256, MX_BK = 128;
constexpr int MX_OPER = MX_BM * MX_BK;            // one operand's 256 rows of a K-step: 32 KB
constexpr int MX_SCALES = (MX_BM + MX_BN) * 4;    // a K-step's scale dwords, A rows then W rows
constexpr int MX_SLOT = 2 * MX_OPER + MX_SCALES;  // 66 KB

template <int EPI>
__global__ __launch_bounds__(512, 1) void gemm_mx_kernel(MxGemmArgs p) {
    static_assert(epi_resid(EPI), "fc2: a residual-stream producer");
    __shared__ __attribute__((aligned(16))) uint8_t smem[2 * MX_SLOT];
    const GemmArgs &a = p.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wc = wave & 3;
    const int g = lane >> 4, li = lane & 15;
    int tm, tn;
    pp_tile_coords(a, (a.M + MX_BM - 1) / MX_BM, xcd_remap(blockIdx.x, gridDim.x), tm, tn);
    const int m0 = tm * MX_BM, n0 = tn * MX_BN;
    const int K = a.K, SB = K / 32, nk = K / MX_BK;
    const int mlast = a.M - 1 - m0;  // last valid tile row: rows past it re-read it (never stored)
    const uint8_t *Ag = p.A8 + (int64_t)m0 * K, *Wg = p.W8 + (int64_t)n0 * K;

    // A K-step is 64 pieces of 1 KB (8 rows x 128 B; A: 0-31, W: 32-63), wave w owns pieces
    // w + 8 i: lane l brings source chunk (l & 7) ^ swizzle of row l >> 3 to LDS bytes [16 l, +16).
    // Then the scale dwords: waves 0-3 the A rows 64 w + l, waves 4-7 the W rows 64 (w - 4) + l.
    uint32_t soff[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = (wave + 8 * (i & 3)) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        soff[i] = (uint32_t)((i < 4 ? min(r, mlast) : r) * K + c * 16);
    }
    const int sr = (wave & 3) * 64 + lane;
    const uint8_t *sg = wave < 4 ? p.As + ((int64_t)m0 + min(sr, mlast)) * SB : p.Ws + ((int64_t)n0 + sr) * SB;
    auto stage = [&](int slot, int kt) {
        uint8_t *base = smem + slot * MX_SLOT;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int piece = wave + 8 * (i & 3);
            // the activation rows stream through once: nontemporal (aux 2), as the bf16 fc2's A
            if (i < 4)
                __builtin_amdgcn_global_load_lds((const void *)(Ag + soff[i] + kt * MX_BK), (lds_void_t *)(base + piece * 1024), 16, 0, 2);
            else
                __builtin_amdgcn_global_load_lds((const void *)(Wg + soff[i] + kt * MX_BK),
                                                 (lds_void_t *)(base + MX_OPER + piece * 1024), 16, 0, 0);
        }
        __builtin_amdgcn_global_load_lds((const void *)(sg + kt * 4), (lds_void_t *)(base + 2 * MX_OPER + wave * 256), 4, 0, 0);
    };
    // fragment of row r0 + li (r0 % 16 == 0): K bytes [16 g, +16) and [64 + 16 g, +16), chunks g and 4 + g
    const int sw = (li >> 1) & 7;
    const int f0 = li * 128 + ((g ^ sw) << 4), f1 = li * 128 + (((4 + g) ^ sw) << 4);
    auto frag = [&](const uint8_t *rows16) {
        const i32x4 lo = *reinterpret_cast<const i32x4 *>(rows16 + f0);
        const i32x4 hi = *reinterpret_cast<const i32x4 *>(rows16 + f1);
        return (i32x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    stage(0, 0);
#pragma nounroll
    for (int kt = 0; kt < nk; ++kt) {
        // this slot's DMA has landed (every wave's, after the barrier), and every wave's fragment
        // reads of the other slot (K-step kt - 1) have returned: it is free for K-step kt + 1
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
        const uint8_t *As = smem + (kt & 1) * MX_SLOT;
        const uint8_t *Ws = As + MX_OPER;
        const uint32_t *Sc = reinterpret_cast<const uint32_t *>(As + 2 * MX_OPER);
        i32x8 wf[4];
        int ws[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            wf[ni] = frag(Ws + (wc * 64 + ni * 16) * 128);
            ws[ni] = (int)(Sc[MX_BM + wc * 64 + ni * 16 + li] >> (8 * g));
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) {
            const i32x8 af = frag(As + (grp * 128 + mi * 16) * 128);
            const int as = (int)(Sc[grp * 128 + mi * 16 + li] >> (8 * g));
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[ni], af, acc[mi][ni], 0, 0, 0, ws[ni], 0, as);
        }
        __builtin_amdgcn_s_setprio(0);
    }
    // the residual producer's epilogue, from the accumulators (no LDS): this wave's 128 rows
    w2_epilogue<EPI, 8, true>(a, acc, smem, m0 + grp * 128, n0, wc);
}

// fc2 of a full batch in MXFP8; a.g.resid_bf16 picks the stream (bf16 under the LayerNorm fold)
inline void launch_gemm_mx(const MxGemmArgs &p_in, hipStream_t s) {
    MxGemmArgs p = p_in;
    RC_REQUIRE(p.g.K % MX_BK == 0 && p.g.K >= MX_BK && p.g.N % MX_BN == 0 && p.g.M >= 1, RC_ERR_INVALID,
               "MXFP8 GEMM: K % 128 == 0, N % 256 == 0");
    RC_REQUIRE(p.g.ln_stats == nullptr || p.g.N == 64 * LN_PARTS, RC_ERR_UNSUPPORTED, "LayerNorm fold needs N = 768");
    RC_REQUIRE(p.g.resid_bf16 ? p.g.ln_x != nullptr : p.g.out_f32 != nullptr, RC_ERR_UNSUPPORTED,
               "the residual stream: ln_x (bf16 stream) or out_f32");
    p.g.group_m = 0;  // row-major tiles: a row tile's three column tiles run together, as the bf16 fc2
    const dim3 gr((p.g.M + MX_BM - 1) / MX_BM * (p.g.N / MX_BN));
    if (p.g.resid_bf16) hipLaunchKernelGGL(gemm_mx_kernel<EPI_RESID_BF16>, gr, dim3(512), 0, s, p);
    else hipLaunchKernelGGL(gemm_mx_kernel<EPI_RESID_F32>, gr, dim3(512), 0, s, p);
    RC_LAUNCH_CHECK();
}

// fc1 of a full batch with the MXFP8 epilogue (pp_epilogue): the ping-pong kernel only.  out:
// [round_up(M, 256)][N] bytes, then [round_up(M, 256)][N / 32] scale bytes.
template <int EPI>
void launch_gemm_mx_out(const GemmArgs &a_in, hipStream_t s) {
    static_assert(epi_mx(EPI), "the MXFP8 epilogues");
    GemmArgs a = a_in;
    RC_REQUIRE(a.K % 64 == 0 && a.K >= 64 && a.N % 256 == 0 && a.M > 256 && a.ldc == 0, RC_ERR_UNSUPPORTED,
               "MXFP8 epilogue: the tiled kernel (M > 256), K % 64 == 0, N % 256 == 0, dense rows");
    if constexpr (epi_ln(EPI)) RC_REQUIRE(a.ln_c && a.ln_stats, RC_ERR_UNSUPPORTED, "LayerNorm-fold consumer needs ln_c and ln_stats");
    a.group_m = gemm_group_m(a);
    launch_pp<EPI, 0, PP_BM>(a, (a.M + PP_BM - 1) / PP_BM, s);
    RC_LAUNCH_CHECK();
}

}  // namespace rc
