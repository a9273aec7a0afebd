// gemm_skinny.h — the GEMMs for M <= 256 rows (a lone image's 70-kernel chain, the CLS rows of
// the last layer): gemm_skinny_kernel, gemm_skinny_shared_kernel, gemm_skinny_ln_kernel,
// gemm_skinny_splitk_kernel + skinny_reduce_kernel, patch_skinny_kernel.  A wave owns 16 rows x
// 32 columns over the whole K and runs the MFMAs in the k order of the tiled kernels, so a row
// gets the same bits here as there.  Part of gemm.h (which includes it: GemmArgs, the epilogue
// helpers and with_k_tiles come from there); the launchers that choose these kernels stay in gemm.h.
#pragma once

#include "vit_kernels.h"

namespace rc {

// The skinny kernels' K chain: nk steps of 32, acc[ni] += W[ni]·A in k order (one dependent
// 16x16x32 MFMA per step, the order of every tiled kernel: the same bits), with the operands of
// the next D steps in flight in a register ring, so the chain waits for one step's loads while
// D − 1 more are on their way (a lone image's GEMMs are latency-bound: 197 rows give 300-1250
// waves for 1024 SIMDs).  NK > 0: the step count is a constant and the chain is straight-line
// code — in a loop the wait-count pass falls back to vmcnt(0) at the loop head, one full memory
// latency per trip.  NK = 0: any even nk, a 2-deep ring in a loop.
template <int NI, int NK, int D>
__device__ __forceinline__ void skinny_chain_t(const uint16_t *Ar, const uint16_t *Wr, int K, int nk, f32x4 (&acc)[NI]) {
    bf16x8 ra[D], rw[D][NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < D; ++d) {
        ra[d] = *reinterpret_cast<const bf16x8 *>(Ar + 32 * d);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) rw[d][ni] = *reinterpret_cast<const bf16x8 *>(Wr + (int64_t)ni * 16 * K + 32 * d);
    }
    auto step = [&](int st, bf16x8 &a_, bf16x8 (&w_)[NI], bool more) __attribute__((always_inline)) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w_[ni], a_, acc[ni], 0, 0, 0);
        if (more) {
            const int kn = 32 * (st + D);
            a_ = *reinterpret_cast<const bf16x8 *>(Ar + kn);
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) w_[ni] = *reinterpret_cast<const bf16x8 *>(Wr + (int64_t)ni * 16 * K + kn);
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the ring: no load hoisted or sunk across steps
    };
    if constexpr (NK > 0) {
        static_assert(NK % D == 0, "ring depth divides the step count");
#pragma unroll
        for (int st = 0; st < NK; ++st) step(st, ra[st % D], rw[st % D], st + D < NK);
    } else {
        for (int kb = 0; kb < nk; kb += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) step(kb + d, ra[d], rw[d], kb + d + D < nk);
        }
    }
}

// ------------------------------------------------------------ the LDS-DMA ring K chain --
// The skinny K chain through an LDS-DMA ring (K = 768 / 3072, and the patch embedding's 768): per
// 64-deep K block a wave copies whole rows, 128 B each, with global_load_lds_dwordx4 — 8 whole rows
// per instruction (8 full 128-B lines) where the register form's fragment loads touch 16 rows × 64 B
// (16 half lines) per instruction: the loads are address-bound (PMC), the bytes are not.  Rows
// are 128 B in LDS with the 16-B chunk XOR-swizzled by (row >> 1) & 7 on the source address
// (conflict-free ds_read_b128 fragments, as the tiled kernels).  The ring is SK stages deep (the
// copy of block kb + SK − 1 issued while block kb is consumed).  A counted vmcnt says the wave's
// own copies of a block have landed, and its fragments are read with inline-asm ds_reads behind one
// lgkmcnt(0) tied to them (as C++ loads hipcc would wait for the whole DMA ring first).  The
// stage block kb − 1 used is refilled BEFORE block kb's MFMAs, so the copy flies under them.  The
// order of these volatile statements is the schedule: wait, (barrier,) reads, tied wait, refill,
// MFMAs.  The MFMAs run in the same k order as every other kernel: the same bits.
//
// One loop, skinny_ring_chain, for two stage layouts (what a wave copies and where its
// fragments lie):
//   own     one wave per ring (gemm_skinny_kernel, gemm_skinny_ln_kernel): per stage its 16 A rows
//           (rows past M: clamped), then its 32 W rows; no barrier.
//   SHARED  SKR waves per ring (gemm_skinny_shared_kernel): each wave copies its own 16 A rows (to
//           wave·2048) and a quarter of the 32 W rows (at SKR·2048), and reads all 32.  One barrier
//           per K block behind the counted wait: it says every wave's copies of block kb have
//           landed and that every wave has read block kb − 1, whose stage is then refilled.
// patch_skinny_kernel runs the own form without the A half (A fragments in registers) and keeps
// that loop in its body: see there.
constexpr int SKINNY_DMA_STAGES = 6;
// fc1 on the one-wave kernel keeps 5 stages: 30 KB of LDS per wave puts five waves on a CU (measured
// on a lone image's 1 248 fc1 tiles, before gemm_skinny_shared_kernel took them: six stages left a
// second round of 224 blocks; device time 436 -> 419 us, profiles/r06/r06ae_skinny_ring_depth_b1_ab.log).
// Deeper rings for the two-wave LayerNorm producers (10 stages) and five for QKV measured no better.
constexpr int SKINNY_FC1_STAGES = 5;

// s_waitcnt vmcnt(younger · X) for a wave that issues X copies per K block: the copies retire in
// order, so a block has landed once only the `younger` blocks behind it are in flight.  The count
// is an immediate: `younger` is a constant after unrolling and one arm survives.
template <int X>
__device__ __forceinline__ void skinny_wait_younger(int younger) {
    static_assert(9 * X <= 63, "every arm's count fits the 6-bit vmcnt field");
    if (younger >= 9) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(9 * X) : "memory");
    else if (younger == 8) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 * X) : "memory");
    else if (younger == 7) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(7 * X) : "memory");
    else if (younger == 6) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(6 * X) : "memory");
    else if (younger == 5) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(5 * X) : "memory");
    else if (younger == 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * X) : "memory");
    else if (younger == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * X) : "memory");
    else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * X) : "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(X) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

constexpr int SKR = 4;  // SHARED: row tiles (waves) per ring
constexpr int skinny_ring_stage_bytes(bool shared) { return ((shared ? SKR * 16 : 16) + 32) * 128; }

// acc[ni] = Σ over NKB blocks of 64 of W[n0 + 16 ni + li]·A[row_a0 + li] through `ring` (SK stages);
// wave: the wave in its block (SHARED).  The set-up differs per layout, the loop does not.
template <bool SHARED, int NKB, int SK>
__device__ __forceinline__ void skinny_ring_chain(const uint16_t *__restrict__ A, int row_a0, int M, const uint16_t *__restrict__ W,
                                                  int n0, int K, uint8_t *ring, int wave, f32x4 (&acc)[2]) {
    constexpr int NI = 2, SB = skinny_ring_stage_bytes(SHARED), WOFF = SKR * 2048;
    constexpr int NP = SHARED ? 3 : 2 + 2 * NI;  // copies per wave and K block
    static_assert(NKB >= SK, "the ring is primed with SK - 1 blocks");
    static_assert((SK - 1) * NP <= 63 && SK <= 11, "the copies in flight fit the 6-bit vmcnt, at most 9 younger blocks");
    const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
    // copy i moves 8 rows, 8 lanes each (row r of its block, source chunk lane % 8 swizzled), to stage byte dst[i]
    const uint16_t *src[NP];
    uint32_t dst[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if constexpr (!SHARED) {  // A rows 8 i + lane / 8 (i < 2), then W rows 8 (i - 2) + lane / 8: piece i
            const int r = (i < 2 ? i : i - 2) * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((r >> 1) & 7);
            const uint16_t *rowp = i < 2 ? A + (int64_t)min(row_a0 + r, M - 1) * K : W + (int64_t)(n0 + r) * K;
            src[i] = rowp + c * 8;
            dst[i] = i * 1024;
        } else {  // i = 0, 1: the wave's A rows; i = 2: W row 8·wave + lane / 8
            const int r = i < 2 ? i * 8 + (lane >> 3) : wave * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((r >> 1) & 7);
            src[i] = (i < 2 ? A + (int64_t)min(row_a0 + r, M - 1) * K : W + (int64_t)(n0 + r) * K) + c * 8;
            dst[i] = i < 2 ? (uint32_t)(wave * 2048 + i * 1024) : (uint32_t)(WOFF + wave * 1024);
        }
    }
    auto issue = [&](int kb) __attribute__((always_inline)) {
        uint8_t *st = ring + (kb % SK) * SB;
#pragma unroll
        for (int i = 0; i < NP; ++i)
            __builtin_amdgcn_global_load_lds((const void *)(src[i] + kb * 64), (lds_void_t *)(st + dst[i]), 16, 0, 0);
    };
    // fragment addresses within a stage: A row li, W row 16 ni + li; logical chunk 4 s + g
    uint32_t fa[2], fw[2][NI];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        const int c = (4 * s2 + g) ^ ((li >> 1) & 7);
        if constexpr (!SHARED) fa[s2] = (uint32_t)(li * 128 + c * 16);
        else fa[s2] = (uint32_t)(wave * 2048 + li * 128 + c * 16);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            if constexpr (!SHARED) fw[s2][ni] = (uint32_t)((16 + 16 * ni + li) * 128 + c * 16);
            else fw[s2][ni] = (uint32_t)(WOFF + (16 * ni + li) * 128 + c * 16);
        }
    }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < SK - 1; ++kb) issue(kb);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        // block kb landed: younger copies in flight are those of blocks kb + 1 .. min(kb + SK - 2, NKB - 1)
        skinny_wait_younger<NP>(min(SK - 2, NKB - 1 - kb));
        if constexpr (SHARED) {
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        const uint32_t st = (uint32_t)(uintptr_t)(ring + (kb % SK) * SB);
        bf16x8 a[2], w[2][NI];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            asm volatile("ds_read_b128 %0, %1" : "=v"(a[s2]) : "v"(st + fa[s2]));
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) asm volatile("ds_read_b128 %0, %1" : "=v"(w[s2][ni]) : "v"(st + fw[s2][ni]));
        }
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(a[0]), "+v"(a[1]), "+v"(w[0][0]), "+v"(w[0][1]), "+v"(w[1][0]), "+v"(w[1][1]));
        // the stage block kb - 1 used is free (its reads retired a block ago; SHARED: every wave
        // passed this block's barrier after them): refill it
        if (kb + SK - 1 < NKB) issue(kb + SK - 1);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[s2][ni], a[s2], acc[ni], 0, 0, 0);
    }
}

// K (per chain) 768 / 3072: straight-line chains; otherwise the looped form (K % 64 == 0)
template <int NI, int KT>
__device__ __forceinline__ void skinny_chain(const uint16_t *Ar, const uint16_t *Wr, int K, int nk, f32x4 (&acc)[NI]) {
    if constexpr (KT > 0) skinny_chain_t<NI, KT / 32, 12>(Ar, Wr, K, nk, acc);
    else skinny_chain_t<NI, 0, 2>(Ar, Wr, K, nk, acc);
}

// Skinny GEMM for M <= 256 (the last layer's CLS rows: O-proj, fc1, fc2 with
// M = images in the slice).  A 256-row tile kernel would put the whole launch on
// N/256 CUs with the full K loop on each (fc2: 3 CUs x 3072-deep); here every
// wave owns 16 rows x 16·NI columns over the whole K, operands straight from
// global memory (W is 1.2-4.7 MB, L2-resident after the first row tile), so the
// launch spreads over ceil(M/16)·N/(16·NI) waves.  Swapped operands as in the
// tiled kernels: the A-operand is 16 weight rows, so lane (g, li) ends with
// activation row li, output columns 4g..4g+3 of each 16-column group.
// Block b runs on XCD b % 8; skinny_block(b) numbers the blocks so that each XCD gets one
// contiguous range (bijective), and tiles are numbered column-major — so the waves of a block
// (consecutive row tiles of one column tile) read the same weight rows at about the same time
// (L1 hits), and a column tile's weights are fetched into one XCD's L2 only (W is re-read by
// every row tile: 13x for a lone image's 197 rows).
__device__ __forceinline__ int skinny_block(int b, int nwg) {
    const int q8 = nwg / 8, r8 = nwg % 8, xcd = b % 8;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + b / 8;
}

// The skinny kernels' epilogue (not the LayerNorm producers): lane (g, li) holds row `row`, columns
// n0 + 16 ni + 4g .. + 3 of acc[ni]
template <int EPI, int NI>
__device__ __forceinline__ void skinny_epilogue(const GemmArgs &a, const f32x4 (&acc)[NI], int row, int n0, int g) {
    float2 lrs;  // LayerNorm fold: this row's (rstd, -rstd*mu), as gemm_pp_kernel computes it
    if constexpr (epi_ln(EPI)) lrs = ln_row_scale(a.ln_stats + (int64_t)row * LN_STRIDE, a.ln_eps);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const int c = n0 + ni * 16 + 4 * g;
        const float4 b = *reinterpret_cast<const float4 *>(a.bias + c);
        float v0, v1, v2, v3;
        if constexpr (epi_ln(EPI)) {
            const float4 v = ln_apply4(lrs, acc[ni], *reinterpret_cast<const float4 *>(a.ln_c + c), b);
            v0 = v.x, v1 = v.y, v2 = v.z, v3 = v.w;
        } else {
            v0 = acc[ni][0] + b.x, v1 = acc[ni][1] + b.y, v2 = acc[ni][2] + b.z, v3 = acc[ni][3] + b.w;
        }
        if constexpr (EPI == EPI_RESID_BF16) {  // residual stream in bf16 (LN producers: gemm_skinny_ln_kernel)
            const int64_t off = (int64_t)row * a.N + c;
            const float4 r = rs_load4(a.ln_x + off);
            rs_store4(make_float4(v0 + r.x, v1 + r.y, v2 + r.z, v3 + r.w), a.ln_x + off, true);
        } else if constexpr (EPI == EPI_RESID_F32) {
            float4 *o = reinterpret_cast<float4 *>(a.out_f32 + (int64_t)row * a.N + c);
            const float4 r = *o;
            *o = make_float4(r.x + v0, r.y + v1, r.z + v2, r.w + v3);
        } else {
            if constexpr (epi_gelu(EPI)) {
                const f32x2 lo = gelu_fast2(f32x2{v0, v1}), hi = gelu_fast2(f32x2{v2, v3});
                v0 = lo.x;
                v1 = lo.y;
                v2 = hi.x;
                v3 = hi.y;
            }
            *reinterpret_cast<uint2 *>(a.out_bf16 + (int64_t)row * (a.ldc ? a.ldc : a.N) + c) =
                make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
        }
    }
}

// One wave per block: the loads are address-bound (PMC: the texture addresser busy for the
// whole launch on the CUs holding blocks), so a tile per CU where 4-wave blocks put four.
// (Two or four tiles per block, one wave and one DMA ring each, the same bits: 423.6 / 431.0 vs
// 427.0 us of device time per one-image request, profiles/r06/r06j_skinny_wpb_ab.log.)
template <int EPI, int NI, int KT, int SK = SKINNY_DMA_STAGES>
__global__ __launch_bounds__(64) void gemm_skinny_kernel(GemmArgs a) {
    const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
    const int nct = a.N / (16 * NI), nrt = (a.M + 15) / 16;
    const int w = skinny_block(blockIdx.x, gridDim.x);
    if (w >= nct * nrt) return;
    const int ct = w / nrt, rt = w % nrt;
    const int K = a.K, n0 = ct * 16 * NI, row = rt * 16 + li;
    f32x4 acc[NI];
    if constexpr (KT > 0) {
        __shared__ __attribute__((aligned(16))) uint8_t ring[SK * skinny_ring_stage_bytes(false)];
        skinny_ring_chain<false, KT / 64, SK>(a.A, rt * 16, a.M, a.W, n0, K, ring, 0, acc);
    } else {
        const uint16_t *Ar = a.A + (int64_t)min(row, a.M - 1) * K + 8 * g;  // rows past M: clamped loads, no stores
        const uint16_t *Wr = a.W + (int64_t)(n0 + li) * K + 8 * g;
        skinny_chain<NI, KT>(Ar, Wr, K, K / 32, acc);
    }
    if (row >= a.M) return;
    skinny_epilogue<EPI, NI>(a, acc, row, n0, g);
}

// Weights shared by SKR row tiles (QKV / fc1 of a lone image, K = 768 / 3072): a block of SKR waves
// owns SKR consecutive 16-row tiles of one 32-column tile; per 64-deep K block each wave copies its
// own 16 A rows and a quarter of the 32 W rows into one LDS stage, and every wave reads all 32 W rows
// from it — W crosses L2 -> CU once per row group instead of once per row tile (a one-image fc1
// moved 61 MB of W for 4.7 MB of unique weights): skinny_ring_chain's SHARED layout.
// Waves of a row group past M copy clamped rows and skip the stores.
// grid: (N / 32) · ceil(ceil(M / 16) / SKR) blocks of SKR waves, column-tile-major through skinny_block
template <int EPI, int KT, int SK = SKINNY_DMA_STAGES>
__global__ __launch_bounds__(64 * SKR) void gemm_skinny_shared_kernel(GemmArgs a) {
    constexpr int NI = 2;
    const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nct = a.N / 32, nrt = (a.M + 15) / 16, nrg = (nrt + SKR - 1) / SKR;
    const int b = skinny_block(blockIdx.x, gridDim.x);
    if (b >= nct * nrg) return;  // block-uniform
    const int ct = b / nrg, rt = (b % nrg) * SKR + wave;
    const int n0 = ct * 32, row = rt * 16 + li;
    __shared__ __attribute__((aligned(16))) uint8_t ring[SK * skinny_ring_stage_bytes(true)];
    f32x4 acc[NI];
    skinny_ring_chain<true, KT / 64, SK>(a.A, rt * 16, a.M, a.W, n0, a.K, ring, wave, acc);
    if (row >= a.M) return;
    skinny_epilogue<EPI, NI>(a, acc, row, n0, g);
}

// LayerNorm block partials of the two-wave producers (gemm_skinny_ln_kernel, patch_skinny_kernel):
// both waves have put the value each element of the block's 16 rows x 64 columns now stands for
// into xs_l (row pitch SKINNY_LN_PITCH floats).  Called by wave 0 after the block's barrier (both
// stay with the kernel: a `return` in here would not end it): the wave reads the 16 rows'
// canonical slices (4 lanes per row), reduces them with ln_block_reduce_quad and stores row
// 16 rt + r's partial of column block blk at row stats_row(16 rt + r) of a.ln_stats.
constexpr int SKINNY_LN_PITCH = 68;
template <typename RowMap>
__device__ __forceinline__ void skinny_ln_partials(const GemmArgs &a, const float *xs_l, int lane, int rt, int blk, RowMap stats_row) {
    constexpr int LP = SKINNY_LN_PITCH;
    const int r = lane >> 2, sg = lane & 3;
    float xs[16];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float *q = xs_l + r * LP + ln_slice_col(sg, c);
        const float4 u = *reinterpret_cast<const float4 *>(q), v = *reinterpret_cast<const float4 *>(q + 4);
        xs[8 * c] = u.x, xs[8 * c + 1] = u.y, xs[8 * c + 2] = u.z, xs[8 * c + 3] = u.w;
        xs[8 * c + 4] = v.x, xs[8 * c + 5] = v.y, xs[8 * c + 6] = v.z, xs[8 * c + 7] = v.w;
    }
    const float2 st = ln_block_reduce_quad(ln_slice_stats(xs), sg);
    const int srow = rt * 16 + r;
    if (sg == 0 && srow < a.M) *reinterpret_cast<float2 *>(a.ln_stats + stats_row(srow) * LN_STRIDE + 2 * blk) = st;
}

// The skinny GEMM as a LayerNorm-fold producer (residual epilogues with ln_x + ln_stats, N = 768:
// O-proj / fc2 of a batch of one image, the CLS O-proj): the block-partial statistics are
// computed in the epilogue (the canonical slices and reduction tree of every producer, bit for bit;
// round 4 ran them as a second launch, 5 us each at batch 1).
// A block of 2 waves owns one row tile × one 64-column LayerNorm block (blocks numbered column-
// block-major through skinny_block: a column block's weights stay in one XCD): wave w computes
// rows 16·rt + li, columns 64·blk + 32·w + 16·ni + 4g + e (the skinny kernel's tile and K chain),
// stores as gemm_skinny_kernel does and puts the value each element now stands for (the stored
// f32 or bf16) into LDS for skinny_ln_partials.  (4-wave blocks of two row tiles: 84 blocks for a
// lone image's fc2, address-bound on 84 CUs at 34 us.)
template <int EPI, int KT>
__global__ __launch_bounds__(128) void gemm_skinny_ln_kernel(GemmArgs a) {
    static_assert(epi_resid(EPI), "LayerNorm producers are residual epilogues");
    constexpr int NI = 2, LP = SKINNY_LN_PITCH;
    __shared__ float xs_l[16 * LP];
    const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15, wave = threadIdx.x >> 6;
    const int nrt = (a.M + 15) / 16, lb = skinny_block(blockIdx.x, gridDim.x);
    const int blk = lb / nrt, rt = lb % nrt;  // column-block-major (skinny_block)
    const int K = a.K, n0 = blk * 64 + wave * 32, row = rt * 16 + li;
    f32x4 acc[NI];
    if constexpr (KT > 0) {
        __shared__ __attribute__((aligned(16))) uint8_t ring[2][SKINNY_DMA_STAGES * skinny_ring_stage_bytes(false)];
        skinny_ring_chain<false, KT / 64, SKINNY_DMA_STAGES>(a.A, rt * 16, a.M, a.W, n0, K, ring[wave], 0, acc);
    } else {
        const uint16_t *Ar = a.A + (int64_t)min(row, a.M - 1) * K + 8 * g;
        const uint16_t *Wr = a.W + (int64_t)(n0 + li) * K + 8 * g;
        skinny_chain<NI, KT>(Ar, Wr, K, K / 32, acc);
    }
    const bool valid = row < a.M;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const int c = n0 + ni * 16 + 4 * g;
        const float4 b = *reinterpret_cast<const float4 *>(a.bias + c);
        const float v0 = acc[ni][0] + b.x, v1 = acc[ni][1] + b.y, v2 = acc[ni][2] + b.z, v3 = acc[ni][3] + b.w;
        const int64_t off = (int64_t)min(row, a.M - 1) * a.N + c;
        float4 x;
        if constexpr (EPI == EPI_RESID_BF16) {
            const float4 r = rs_load4(a.ln_x + off);
            x = rs_store4(make_float4(v0 + r.x, v1 + r.y, v2 + r.z, v3 + r.w), a.ln_x + off, valid);
        } else {
            float4 *o = reinterpret_cast<float4 *>(a.out_f32 + off);
            const float4 r = *o;
            x = make_float4(r.x + v0, r.y + v1, r.z + v2, r.w + v3);
            if (valid) {
                *o = x;
                *reinterpret_cast<uint2 *>(a.ln_x + off) = pack_bf16x4(x);
            }
        }
        *reinterpret_cast<float4 *>(xs_l + li * LP + wave * 32 + ni * 16 + 4 * g) = x;
    }
    __syncthreads();
    if (wave != 0) return;
    skinny_ln_partials(a, xs_l, lane, rt, blk, [](int srow) { return (int64_t)srow; });
}

// Split-K skinny GEMM with an f32 residual epilogue, for the last layer's fc2 on the
// CLS rows (M = images, N = 768, K = 3072; every batch size, so the CLS rows of an image
// get the same bits in any batch): the skinny kernel's one wave per 16
// rows x 32 columns walks all of K as a chain of dependent 16x16x32 MFMAs and global
// loads (54 us at M = 128); here KS waves split K, write f32 partials [KS][M][N], and
// skinny_reduce_kernel adds them in ks order + bias + the residual (deterministic).
// Used only on the CLS rows, so batch invariance is unaffected (the full-layer GEMMs of
// a small batch keep the skinny kernel, bit-identical to the tiled ones).
template <int NI, int KS, int KT>
__global__ __launch_bounds__(64) void gemm_skinny_splitk_kernel(GemmArgs a, float *__restrict__ part) {
    const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
    const int nct = a.N / (16 * NI), nrt = (a.M + 15) / 16;
    const int w = blockIdx.x;  // one wave per block (address-bound loads: spread over CUs)
    if (w >= nct * nrt * KS) return;
    const int ks = w % KS, tile = w / KS;
    const int ct = tile % nct, rt = tile / nct;
    const int KL = a.K / KS, k0 = ks * KL;
    const int n0 = ct * 16 * NI, row = rt * 16 + li;
    const uint16_t *Ar = a.A + (int64_t)min(row, a.M - 1) * a.K + k0 + 8 * g;
    const uint16_t *Wr = a.W + (int64_t)(n0 + li) * a.K + k0 + 8 * g;
    f32x4 acc[NI];
    skinny_chain<NI, KT>(Ar, Wr, a.K, KL / 32, acc);
    if (row >= a.M) return;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
        *reinterpret_cast<f32x4 *>(part + ((int64_t)ks * a.M + row) * a.N + n0 + ni * 16 + 4 * g) = acc[ni];
}

template <int KS>
__global__ __launch_bounds__(256) void skinny_reduce_kernel(GemmArgs a, const float *__restrict__ part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one float4 of outputs
    if (i >= (int64_t)a.M * a.N / 4) return;
    const int64_t e = i * 4;
    const int c = (int)(e % a.N);
    float4 s = *reinterpret_cast<const float4 *>(part + e);
#pragma unroll
    for (int ks = 1; ks < KS; ++ks) {
        const float4 p = *reinterpret_cast<const float4 *>(part + (int64_t)ks * a.M * a.N + e);
        s = make_float4(s.x + p.x, s.y + p.y, s.z + p.z, s.w + p.w);
    }
    const float4 b = *reinterpret_cast<const float4 *>(a.bias + c);
    float4 *o = reinterpret_cast<float4 *>(a.out_f32 + e);
    const float4 r = *o;
    *o = make_float4(r.x + (s.x + b.x), r.y + (s.y + b.y), r.z + (s.z + b.z), r.w + (s.w + b.w));
}

constexpr int SKINNY_KS = 4;

// out_f32 [M][N] += A·Wᵀ + bias on the split-K skinny path (part: >= SKINNY_KS·M·N floats)
inline void launch_skinny_splitk_resid(const GemmArgs &a, float *part, hipStream_t s) {
    RC_REQUIRE(a.M >= 1 && a.N % 32 == 0 && a.K % (32 * SKINNY_KS) == 0 && a.out_f32 && !a.ln_x, RC_ERR_UNSUPPORTED,
               "split-K skinny GEMM: N % 32 == 0, K % 128 == 0, f32 residual");
    const int waves = ((a.M + 15) / 16) * (a.N / 32) * SKINNY_KS;
    with_k_tiles<768>(a.K / SKINNY_KS, [&](auto kt) {  // K per chain
        hipLaunchKernelGGL((gemm_skinny_splitk_kernel<2, SKINNY_KS, decltype(kt)::value>), dim3(waves), dim3(64), 0, s, a, part);
    });
    RC_LAUNCH_CHECK();
    const int64_t n4 = (int64_t)a.M * a.N / 4;
    hipLaunchKernelGGL(skinny_reduce_kernel<SKINNY_KS>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, a, part);
    RC_LAUNCH_CHECK();
}

// The patch embedding of a small batch (M <= 256 patch rows, the bf16 stream: one image is
// 196 rows, and patch_gemm_kernel's 128 x 256 tiles put it on 6 workgroups, 33 us): the skinny
// form.  Block = 2 waves = one 16-row tile x one 64-column LayerNorm block (as
// gemm_skinny_ln_kernel); wave w takes columns 32w..32w+31.  A fragments are built in registers
// from the u8 images — lane (g, li), K-step s: patch row 16 rt + li, K = 32 s + 8 g .. + 7 in
// (ky, kx, c) order, 8 bytes of one image row, each bf16(fma(u, pre_a[k mod 3], pre_b[k mod 3]))
// exactly as patch_gemm_kernel converts them — and the W rows stream through the LDS-DMA ring;
// the MFMAs run in the same K order (the same bits).  Epilogue: x = (acc + bias) + position
// embedding at the patch's token row, stored to the bf16 stream, LN partials of the 64-column
// block through LDS (f32_rows_epilogue's values and canonical slices).
template <int EPI>
__global__ __launch_bounds__(128) void patch_skinny_kernel(GemmArgs a) {
    static_assert(EPI == EPI_PATCH_BF16, "the bf16 stream");
    constexpr int NI = 2, P = 16, KC = 3 * P * P, NKB = KC / 64, LP = SKINNY_LN_PITCH;
    constexpr int SK = SKINNY_DMA_STAGES, SB = 16 * NI * 128;
    __shared__ __attribute__((aligned(16))) uint8_t ring[2][SK * SB];
    __shared__ float xs_l[16 * LP];
    const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15, wave = threadIdx.x >> 6;
    const int nrt = (a.M + 15) / 16, lb = skinny_block(blockIdx.x, gridDim.x);
    const int blk = lb / nrt, rt = lb % nrt;
    const int n0 = blk * 64 + wave * 32, row = rt * 16 + li;
    // this lane's patch row: 8 image bytes per K-step, all 24 steps loaded up front
    const int S = a.img_size, gp = S / P, np = gp * gp;
    const int m = min(row, a.M - 1);
    const int b = m / np, pi = m - b * np, py = pi / gp, px = pi - py * gp;
    const uint8_t *abase = a.img + (((int64_t)b * S + py * P) * S + px * P) * 3;
    uint2 ab[2 * NKB];
#pragma unroll
    for (int st = 0; st < 2 * NKB; ++st) {
        const int k0 = 32 * st + 8 * g, ky = k0 / (3 * P), off = k0 - ky * (3 * P);
        ab[st] = *reinterpret_cast<const uint2 *>(abase + ky * S * 3 + off);
    }
    // every A fragment converted up front (24 x 16 B per lane; constant indices below)
    const float pa[3] = {a.pre_a[0], a.pre_a[1], a.pre_a[2]}, pb[3] = {a.pre_b[0], a.pre_b[1], a.pre_b[2]};
    bf16x8 af[2 * NKB];
#pragma unroll
    for (int st = 0; st < 2 * NKB; ++st) {
        const int c0 = (32 * st + 8 * g) % 3;  // channel of byte 0 (k mod 3; 3P = 48 keeps rows aligned)
        // the (a, b) pair of byte e is ((c0 + e) mod 3): rotate once, then constant indices
        const float ra[3] = {c0 == 0 ? pa[0] : (c0 == 1 ? pa[1] : pa[2]), c0 == 0 ? pa[1] : (c0 == 1 ? pa[2] : pa[0]),
                             c0 == 0 ? pa[2] : (c0 == 1 ? pa[0] : pa[1])};
        const float rb[3] = {c0 == 0 ? pb[0] : (c0 == 1 ? pb[1] : pb[2]), c0 == 0 ? pb[1] : (c0 == 1 ? pb[2] : pb[0]),
                             c0 == 0 ? pb[2] : (c0 == 1 ? pb[0] : pb[1])};
        const uint32_t w[2] = {ab[st].x, ab[st].y};
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 2 * j;
            const float uA = (float)((w[e >> 2] >> (8 * (e & 3))) & 0xffu);
            const float uB = (float)((w[(e + 1) >> 2] >> (8 * ((e + 1) & 3))) & 0xffu);
            o[j] = pack_bf16x2(fmaf(uA, ra[e % 3], rb[e % 3]), fmaf(uB, ra[(e + 1) % 3], rb[(e + 1) % 3]));
        }
        af[st] = __builtin_bit_cast(bf16x8, make_uint4(o[0], o[1], o[2], o[3]));
    }
    // W rows n0 .. n0 + 31 by LDS-DMA: skinny_ring_chain's ring and loop without the A half, written
    // out here because as a third layout of that function the compiler schedules this kernel's
    // address arithmetic differently (tools/kernel_asm_diff.py) — keep the two loops in step.
    uint8_t *rg = ring[wave];
    const uint16_t *src[2 * NI];
#pragma unroll
    for (int i = 0; i < 2 * NI; ++i) {
        const int r = i * 8 + (lane >> 3);
        src[i] = a.W + (int64_t)(n0 + r) * KC + (((lane & 7) ^ ((r >> 1) & 7)) * 8);
    }
    auto issue = [&](int kb) __attribute__((always_inline)) {
        uint8_t *stg = rg + (kb % SK) * SB;
#pragma unroll
        for (int i = 0; i < 2 * NI; ++i)
            __builtin_amdgcn_global_load_lds((const void *)(src[i] + kb * 64), (lds_void_t *)(stg + i * 1024), 16, 0, 0);
    };
    uint32_t fw[2][NI];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) fw[s2][ni] = (uint32_t)((16 * ni + li) * 128 + (((4 * s2 + g) ^ ((li >> 1) & 7)) * 16));
    f32x4 acc[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the image bytes (older than every DMA below)
#pragma unroll
    for (int kb = 0; kb < SK - 1; ++kb) issue(kb);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        skinny_wait_younger<2 * NI>(min(SK - 2, NKB - 1 - kb));
        const uint32_t st = (uint32_t)(uintptr_t)(rg + (kb % SK) * SB);
        bf16x8 w[2][NI];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) asm volatile("ds_read_b128 %0, %1" : "=v"(w[s2][ni]) : "v"(st + fw[s2][ni]));
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0][0]), "+v"(w[0][1]), "+v"(w[1][0]), "+v"(w[1][1]));
        if (kb + SK - 1 < NKB) issue(kb + SK - 1);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[s2][ni], af[2 * kb + s2], acc[ni], 0, 0, 0);
    }
    // epilogue: f32_rows_epilogue's values, per element
    const bool valid = row < a.M;
    const int img = m / np, p = m - img * np;
    const int64_t orow = (int64_t)img * a.tokens + 1 + p;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const int c = n0 + ni * 16 + 4 * g;
        const float4 bb = *reinterpret_cast<const float4 *>(a.bias + c);
        const float4 ps = *reinterpret_cast<const float4 *>(a.pos + (int64_t)(1 + p) * a.N + c);
        const float4 xf = make_float4((acc[ni][0] + bb.x) + ps.x, (acc[ni][1] + bb.y) + ps.y, (acc[ni][2] + bb.z) + ps.z,
                                      (acc[ni][3] + bb.w) + ps.w);
        *reinterpret_cast<float4 *>(xs_l + li * LP + wave * 32 + ni * 16 + 4 * g) = rs_store4(xf, a.ln_x + orow * a.N + c, valid);
    }
    if (a.ln_stats == nullptr) return;  // block-uniform
    __syncthreads();
    if (wave != 0) return;
    skinny_ln_partials(a, xs_l, lane, rt, blk, [&](int srow) {  // patch row -> token row
        const int simg = srow / np, sp = srow - simg * np;
        return (int64_t)simg * a.tokens + 1 + sp;
    });
}

}  // namespace rc
