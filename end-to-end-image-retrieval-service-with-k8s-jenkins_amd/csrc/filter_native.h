// filter_native.h — the batched search's native (f16 / bf16) filter kernels and their one host
// dispatch.  Two kernel templates, filter_gemm_kernel and filter_qs_kernel, each with the optional
// compile-time forms METRIC, MASKED and PAGED (filter_mfma.h has the forms' helpers and the
// arguments that make them exact).  search_mfma.hip instantiates the contiguous forms and
// search_mfma_paged.hip the PAGED ones, through launch_filter_native<T, PAGED>.
#pragma once

#include "filter_mfma.h"

namespace rc {

// What both kernels take, by value.  A form that does not read a field leaves it dead.
struct FilterNativeArgs {
    FilterArgs a;
    FilterMetric fm;       // METRIC
    const uint32_t *mask;  // MASKED: [ceil(r_end / 32)], over the local rows (BatchPlan::mask)
    const int32_t *pages;  // PAGED: the namespace's page table (BatchPlan::pages)
};

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
template <typename T, bool METRIC = false, bool MASKED = false, bool PAGED = false>
__global__ __launch_bounds__(512, 1) void filter_gemm_kernel(FilterNativeArgs fa) {
    // (copies, not references into fa: the fields then load as they did as separate kernel parameters)
    const FilterArgs a = fa.a;
    [[maybe_unused]] const FilterMetric fm = fa.fm;
    [[maybe_unused]] const uint32_t *const mask = fa.mask;
    [[maybe_unused]] const int32_t *const pages = fa.pages;
    using Op = MfmaOp<T>;
    using v8 = typename Op::v8;
    constexpr int BK = 64;
    constexpr int A_BYTES = SB_TILE * BK * 2, STAGE = 2 * A_BYTES;
    __shared__ __attribute__((aligned(16))) uint8_t smem[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wc = wave & 3;
    const int g = lane >> 4, li = lane & 15;

    const FilterBlock fb(a, SB_TILE);
    const int qb = fb.qb;
    const int64_t rt0 = fb.rt0, rt1 = fb.rt1;
    if (rt0 >= rt1) return;  // block-uniform
    const int nkt = a.nkt;
    const int64_t ld = a.ld;
    const int64_t nsteps = (rt1 - rt0) * nkt;
    const uint16_t *Ag = (const uint16_t *)a.qh + (int64_t)qb * SB_TILE * ld;
    // PAGED: Rg is the pool's first row; a tile is one whole page, found in stage4
    const uint16_t *Rg = (const uint16_t *)a.rows + (PAGED ? (int64_t)0 : (a.r_begin + rt0 * SB_TILE) * ld);
    // PAGED: the page of the tile being staged (pg_cur) and of the tile after it (pg_ahead, loaded a
    // tile ahead of the loads that need it); pg_epi is the page of the tile whose epilogue comes next
    // (METRIC: its norms), loaded where mw is.  Wave-uniform scalar loads (load_page).
    [[maybe_unused]] const int64_t pos0 = a.r_begin + rt0 * SB_TILE;
    [[maybe_unused]] int32_t pg_cur = 0, pg_ahead = 0, pg_epi = 0;
    if constexpr (PAGED) pg_ahead = load_page(pages, pos0);
    if constexpr (PAGED && METRIC) pg_epi = load_page(pages, pos0);

    // 64 pieces of 1 KB per step (queries: 0-31, rows: 32-63); wave w owns pieces w + 8 i.
    auto stage4 = [&](int buf, int64_t step, int i0) {
        uint8_t *base = smem + buf * STAGE;
        const int64_t rt = step / nkt;
        const int k0 = (int)(step - rt * nkt) * BK;
        const uint16_t *Wg = Rg + rt * SB_TILE * ld;
        if constexpr (PAGED) {
            if (i0 == 4) {  // the call that stages the rows; steps come in order, a tile's first takes the page over
                if (k0 == 0) {
                    pg_cur = pg_ahead;
                    pg_ahead = load_page(pages, pos0 + min(rt + 1, rt1 - rt0 - 1) * SB_TILE);
                }
                Wg = Rg + (int64_t)pg_cur * RC_PAGE_ROWS * ld;
            }
        }
#pragma unroll
        for (int i = i0; i < i0 + 4; ++i) {
            const int piece = wave + 8 * i;
            const bool is_q = i < 4;
            const int r = (is_q ? piece : piece - 32) * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((r >> 1) & 7);
            const uint16_t *src = (is_q ? Ag : Wg) + (int64_t)r * ld + k0 + c * 8;
            __builtin_amdgcn_global_load_lds((const void *)src, (lds_void *)(base + piece * 1024), 16, 0, 0);
        }
    };
    auto bar = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    // thresholds of this lane's 8 query rows: q = qb*256 + grp*128 + mq*64 + mi*16 + li
    float thr[2][4];
#pragma unroll
    for (int mq = 0; mq < 2; ++mq)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) thr[mq][mi] = a.thr[qb * SB_TILE + grp * 128 + mq * 64 + mi * 16 + li];

    f32x4_t acc[2][2][4][2];
    auto zero_acc = [&] {
#pragma unroll
        for (int a0 = 0; a0 < 2; ++a0)
#pragma unroll
            for (int a1 = 0; a1 < 2; ++a1)
#pragma unroll
                for (int a2 = 0; a2 < 4; ++a2)
#pragma unroll
                    for (int a3 = 0; a3 < 2; ++a3) acc[a0][a1][a2][a3] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    };
    zero_acc();
    // MASKED: the bitmap words of this wave's 64 rows of the current row tile (wave-uniform: scalar
    // registers), loaded one tile ahead of the epilogue that reads them
    [[maybe_unused]] uint32_t mw[2];
    if constexpr (MASKED) load_mask_words(mask, a.r_begin + rt0 * SB_TILE + wc * 64, a.r_end, mw);

    stage4(0, 0, 0);
    stage4(0, 0, 4);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bar();
    if (grp == 1) bar();  // stagger: G1 one segment behind

    v8 af[4][2], wf[2][2];  // queries [mi][s], rows [ni][s]
    for (int64_t step = 0; step < nsteps; ++step) {
        const int cur = (int)(step & 1);
        const uint8_t *As = smem + cur * STAGE;
        const uint8_t *Ws = As + A_BYTES;
        const bool more = step + 1 < nsteps;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int mq = p >> 1;
            const int nq = (p == 1 || p == 2);
            if (p == 0 || p == 2) {
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int r = grp * 128 + mq * 64 + mi * 16 + li;
                        const int c = s * 4 + g;
                        af[mi][s] = *reinterpret_cast<const v8 *>(As + r * 128 + ((c ^ ((r >> 1) & 7)) << 4));
                    }
            }
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int r = wc * 64 + nq * 32 + ni * 16 + li;
                    const int c = s * 4 + g;
                    wf[ni][s] = *reinterpret_cast<const v8 *>(Ws + r * 128 + ((c ^ ((r >> 1) & 7)) << 4));
                }
            if (more && p < 2) stage4(cur ^ 1, step + 1, p * 4);
            if (p == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            bar();
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        acc[mq][nq][mi][ni] = Op::mma(wf[ni][s], af[mi][s], acc[mq][nq][mi][ni]);
            __builtin_amdgcn_s_setprio(0);
            bar();
        }

        if ((step + 1) % nkt == 0) {
            // ---- epilogue of row tile rt: lane holds S[q][r .. r+3] for 8 q x 4 r-groups
            const int64_t rt = rt0 + step / nkt;
            const int64_t rbase = a.r_begin + rt * SB_TILE + wc * 64 + 4 * g;
            // MASKED: none of the wave's 64 rows is eligible: no epilogue (wave-uniform)
            if (!MASKED || (mw[0] | mw[1]) != 0u) {
                if constexpr (METRIC) {  // u >= thr[q] (the metric epilogue's comment in filter_mfma.h)
                    const int64_t tile_row = a.r_begin + rt * SB_TILE;  // wave-uniform
                    // (PAGED: the norms sit beside the rows, in the tile's page; `left` stays in positions)
                    const float *tn = fm.norms + (PAGED ? (int64_t)pg_epi * RC_PAGE_ROWS : tile_row);
                    const int left = (int)min<int64_t>(a.r_end - tile_row, (int64_t)SB_TILE);
                    f32x4_t nv[2][2];
#pragma unroll
                    for (int nq = 0; nq < 2; ++nq)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) nv[nq][ni] = load_norms4(tn, wc * 64 + 4 * g + nq * 32 + ni * 16, left);
                    // in place: the accumulators become u, and the test below (its maximum as the
                    // wave-uniform early-out, then per row) is the cosine epilogue's own code on them —
                    // no second copy of the values in registers
#pragma unroll
                    for (int mq = 0; mq < 2; ++mq)
#pragma unroll
                        for (int mi = 0; mi < 4; ++mi) {
                            const int q = qb * SB_TILE + grp * 128 + mq * 64 + mi * 16 + li;
                            const f32x4_t k4 = *reinterpret_cast<const f32x4_t *>(fm.mcoef + 4 * q);
#pragma unroll
                            for (int nq = 0; nq < 2; ++nq)
#pragma unroll
                                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                                    for (int j = 0; j < 4; ++j)
                                        acc[mq][nq][mi][ni][j] = metric_upper(k4, acc[mq][nq][mi][ni][j], nv[nq][ni][j]);
                            if (mi % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // at most 2 queries' constants (8 registers) in flight
                        }
                }
                if constexpr (MASKED) {  // ineligible rows leave the test: mask_ineligible4's comment
#pragma unroll
                    for (int nq = 0; nq < 2; ++nq)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) {
                            const uint32_t e = mw[nq] >> (ni * 16 + 4 * g);  // rows wc·64 + nq·32 + ni·16 + 4g + j: bit j
#pragma unroll
                            for (int mq = 0; mq < 2; ++mq)
#pragma unroll
                                for (int mi = 0; mi < 4; ++mi) acc[mq][nq][mi][ni] = mask_ineligible4(acc[mq][nq][mi][ni], e);
                        }
                }
#pragma unroll
                for (int mq = 0; mq < 2; ++mq)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) {
                        const float t = thr[mq][mi];
                        float m = -INFINITY;
#pragma unroll
                        for (int nq = 0; nq < 2; ++nq)
#pragma unroll
                            for (int ni = 0; ni < 2; ++ni) {
                                const f32x4_t v = acc[mq][nq][mi][ni];
                                m = fmaxf(m, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
                            }
                        if (__ballot(m >= t) == 0) continue;  // wave-uniform: the common case
                        if (m >= t) {
                            const int q = qb * SB_TILE + grp * 128 + mq * 64 + mi * 16 + li;
#pragma unroll
                            for (int nq = 0; nq < 2; ++nq)
#pragma unroll
                                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                                    for (int j = 0; j < 4; ++j) {
                                        const int64_t row = rbase + nq * 32 + ni * 16 + j;
                                        if (acc[mq][nq][mi][ni][j] >= t && row < a.r_end) append_candidate(a, q, row);
                                    }
                        }
                    }
            }
            if constexpr (MASKED)
                load_mask_words(mask, a.r_begin + min(rt + 1, rt1 - 1) * SB_TILE + wc * 64, a.r_end, mw);
            if constexpr (PAGED && METRIC) pg_epi = load_page(pages, a.r_begin + min(rt + 1, rt1 - 1) * SB_TILE);
            zero_acc();
        }
    }
    if (grp == 0) bar();  // balance the stagger barrier
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
//
// ABL (A/B diagnostics, diagnostic builds only; 0 in production): bit0 no DMA in the
// loop, bit1 no MFMA, bit2 no fragment reads (MFMAs on the query registers), bit3 no
// epilogue.  T, NKT and ABL come first: the cosine kernel prints as filter_qs_kernel<f16_t, 8, 0, ...>.
template <typename T, int NKT, int ABL = 0, bool METRIC = false, bool MASKED = false, bool PAGED = false>  // 256 queries per block
__global__ __launch_bounds__(512, 1) void filter_qs_kernel(FilterNativeArgs fa) {
    // (copies, not references into fa: the fields then load as they did as separate kernel parameters)
    const FilterArgs a = fa.a;
    [[maybe_unused]] const FilterMetric fm = fa.fm;
    [[maybe_unused]] const uint32_t *const mask = fa.mask;
    [[maybe_unused]] const int32_t *const pages = fa.pages;
    constexpr int QS_WAVES = 16 / QS_QT;
    constexpr int RF = QS_RT / 16;
    using Op = MfmaOp<T>;
    using v8 = typename Op::v8;
    constexpr int STEP_BYTES = QS_RT * 128;  // 16 KB at QT = 2
    __shared__ __attribute__((aligned(16))) uint8_t smem[QS_NS * STEP_BYTES];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;

    const FilterBlock fb(a, QS_RT);
    const int qb = fb.qb;
    const int64_t rt0 = fb.rt0, rt1 = fb.rt1;
    if (rt0 >= rt1) return;  // block-uniform
    const int64_t ld = a.ld;
    const int ntiles = (int)(rt1 - rt0);  // per-block counters in 32 bits: uniform SALU compares
    const int nsteps = ntiles * NKT;
    // PAGED: Rg is the pool's first row; a tile's rows are found through its page (`issue`)
    const uint16_t *Rg = (const uint16_t *)a.rows + (PAGED ? (int64_t)0 : (a.r_begin + rt0 * QS_RT) * ld);

    // this lane's query fragments for the whole K: qf[qt][kk], kk = 32-wide k chunk
    v8 qf[QS_QT][2 * NKT];
    const int q0 = qb * SB_TILE + wave * 16 * QS_QT;
#pragma unroll
    for (int qt = 0; qt < QS_QT; ++qt)
#pragma unroll
        for (int kk = 0; kk < 2 * NKT; ++kk)
            qf[qt][kk] = *reinterpret_cast<const v8 *>((const uint16_t *)a.qh + (int64_t)(q0 + qt * 16 + li) * ld +
                                                       kk * 32 + g * 8);
    // (METRIC: the NKT 8 form has no register to spare in the K loop — query fragments 128,
    // accumulators 64, the pipelined row fragments — so the metric form keeps nothing per lane
    // across it that the cosine form does not: its thresholds are loaded in each epilogue, and the
    // lane index there and in `issue` comes from v_mbcnt, in volatile asm so that it is not hoisted.
    // Whether that suffices is the register allocator's decision, which nothing here can assert:
    // tools/kernel_resources.py --no-scratch metric fails if a metric kernel uses scratch.)
    float thr[QS_QT];
    if constexpr (!METRIC) {
#pragma unroll
        for (int qt = 0; qt < QS_QT; ++qt) thr[qt] = a.thr[q0 + qt * 16 + li];
    }
    // consume the query loads here, so the compiler's vmcnt waits for them sit
    // before the K loop instead of inside it (where they would drain the DMA ring)
#pragma unroll
    for (int qt = 0; qt < QS_QT; ++qt) {
        if constexpr (!METRIC) asm volatile("" ::"v"(thr[qt]));
#pragma unroll
        for (int kk = 0; kk < 2 * NKT; ++kk) asm volatile("" ::"v"(qf[qt][kk]));
    }

    // step t = (tile, k-step): 2·RF pieces of 1 KB (8 rows x 128 B); wave w issues pieces w + QS_WAVES·i.
    constexpr int PPW = 2 * RF / QS_WAVES;
    uint32_t loff[PPW];  // byte offset of this lane's 16 B within the step's rows
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int r = (wave + QS_WAVES * i) * 8 + (lane >> 3);
        loff[i] = (uint32_t)(r * (int)ld + (((lane & 7) ^ ((r >> 1) & 7)) << 3)) * 2u;
    }
    // PAGED: the page of the tile whose steps are being issued (pg_cur) and of the tile after it
    // (pg_ahead, loaded when the tile before it starts: a whole tile of steps ahead of the descriptor
    // that needs it).  Wave-uniform scalar loads (load_page): scalar registers, no VGPR.
    [[maybe_unused]] const int64_t pos0 = a.r_begin + rt0 * QS_RT;  // the block's first position
    [[maybe_unused]] int32_t pg_cur = 0, pg_ahead = 0;
    if constexpr (PAGED) pg_ahead = load_page(pages, pos0);
    auto issue = [&](int t) {
        const int tile = t / NKT;
        const int ks = (int)(t - tile * NKT);
        uint8_t *base = smem + (int)(t % QS_NS) * STEP_BYTES;
        const uint16_t *src = Rg + (int64_t)tile * QS_RT * ld + ks * 64;
        if constexpr (PAGED) {
            if (ks == 0) {  // steps are issued in order: a tile's first step takes the page over
                pg_cur = pg_ahead;
                pg_ahead = load_page(pages, pos0 + (int64_t)min(tile + 1, ntiles - 1) * QS_RT);
            }
            const int in_page = ((int)(pos0 & (RC_PAGE_ROWS - 1)) + tile * QS_RT) & (RC_PAGE_ROWS - 1);
            src = Rg + ((int64_t)pg_cur * RC_PAGE_ROWS + in_page) * ld + ks * 64;
        }
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)src, (short)0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            // (the builtin's operands kept non-dependent: a template-dependent operand defers
            // its target check to instantiation, where the host pass drops the kernel's stub)
            lds_void *dst = (lds_void *)(base + (wave + QS_WAVES * i) * 1024);
            uint32_t off = loff[i];
            if constexpr (METRIC) {  // loff[i] again, from the lane index: no per-lane offsets held across the K loop
                int ln;
                asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
                const int r = (wave + QS_WAVES * i) * 8 + (ln >> 3);
                off = (uint32_t)(r * (int)ld + (((ln & 7) ^ ((r >> 1) & 7)) << 3)) * 2u;
            }
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst, 16, off, 0, 0, 0);
        }
    };
    // one barrier per SPS = 2 k-steps (nsteps is a multiple): steps t..t+SPS-1 land
    // together, steps t+NS-SPS..t+NS-1 go into the slots freed by t-SPS..t-1; NS - SPS
    // steps in flight
    constexpr int SPS = 2;
    for (int t = 0; t < min(QS_NS - SPS, nsteps); ++t) issue(t);

    f32x4_t acc[RF][QS_QT];
    for (int tile = 0; tile < ntiles; ++tile) {
        // MASKED: the tile's bitmap words (wave-uniform: scalar registers, none of the lane's own),
        // loaded here so that their latency runs under the tile's K loop
        [[maybe_unused]] uint32_t mw[QS_RT / 32];
        if constexpr (MASKED) load_mask_words(mask, a.r_begin + (rt0 + tile) * QS_RT, a.r_end, mw);
        [[maybe_unused]] int32_t pg_epi = 0;  // PAGED METRIC: this tile's page, for its norms (as mw: a scalar register)
        if constexpr (PAGED && METRIC) pg_epi = load_page(pages, a.r_begin + (rt0 + tile) * QS_RT);
#pragma unroll
        for (int rf = 0; rf < RF; ++rf)
#pragma unroll
            for (int qt = 0; qt < QS_QT; ++qt)
                acc[rf][qt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kp = 0; kp < NKT / SPS; ++kp) {
            const int t = tile * NKT + SPS * kp;
            // steps t..t+SPS-1 landed: the NS - 2·SPS younger steps (PPW DMAs each) may be in flight
            static_assert(NKT % SPS == 0 && (QS_NS - 2 * SPS) * PPW < 64, "whole sync groups; vmcnt is 6 bits");
            if (t + QS_NS - SPS - 1 < nsteps) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((QS_NS - 2 * SPS) * PPW) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();  // every wave's DMA of t..t+SPS-1 landed; slots of t-SPS..t-1 are free
            asm volatile("" ::: "memory");
#pragma unroll
            for (int j = QS_NS - SPS; j < QS_NS; ++j)
                if (!(ABL & 1) && t + j < nsteps) issue(t + j);
            // groups of 4 row fragments, (k half kl, k sub-chunk sh, row quarter rh): 4 reads,
            // then their 4·QT MFMAs with counted lgkmcnt waits.  Row r = 16 rf + li: its
            // swizzle (r >> 1) & 7 = (li >> 1) & 7 does not depend on rf.  The SIMD
            // partner wave's MFMAs cover the read latency.
            constexpr int RH = RF / 4, NG = SPS * 2 * RH;
            auto frag_ptr = [&](int gi) {
                const int kl = gi / (2 * RH), sh = (gi / RH) % 2, rh = gi % RH;
                return smem + ((t + kl) % QS_NS) * STEP_BYTES + li * 128 + (((sh * 4 + g) ^ ((li >> 1) & 7)) << 4) +
                       rh * 4 * 2048;
            };
            auto load_group = [&](int gi, v8 *dst) {
                const uint8_t *Sr = frag_ptr(gi);
                const int ks = SPS * kp + gi / (2 * RH), sh = (gi / RH) % 2;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    dst[i] = (ABL & 4) ? qf[i & 1][(ks * 2 + sh + i) % (2 * NKT)]
                                       : *reinterpret_cast<const v8 *>(Sr + i * 2048);
            };
#pragma unroll
            for (int gi = 0; gi < NG; ++gi) {
                const int ks = SPS * kp + gi / (2 * RH), sh = (gi / RH) % 2, rh = gi % RH;
                v8 cur[4];
                load_group(gi, cur);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int qt = 0; qt < QS_QT; ++qt)
                        if constexpr (ABL & 2)
                            asm volatile("" ::"v"(cur[i]));
                        else
                            acc[rh * 4 + i][qt] = Op::mma(cur[i], qf[qt][ks * 2 + sh], acc[rh * 4 + i][qt]);
                __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
            }
        }
        // ---- epilogue of row tile rt0 + tile: candidates s' >= thr[q]
        if constexpr (MASKED) {  // no eligible row in the tile: no epilogue (wave-uniform)
            uint32_t any = 0u;
#pragma unroll
            for (int i = 0; i < QS_RT / 32; ++i) any |= mw[i];
            if (any == 0u) continue;
        }
        [[maybe_unused]] int lq = li, gq = g;  // METRIC: li and g again, from v_mbcnt
        if constexpr (METRIC) {
            int ln;
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
            lq = ln & 15;
            gq = ln >> 4;
        }
        const int64_t rbase = a.r_begin + (rt0 + tile) * QS_RT + 4 * gq;
        // MASKED: ineligible rows of acc[rf][.] leave the test below (mask_ineligible4's comment)
        [[maybe_unused]] auto mask_rows = [&](int rf) __attribute__((always_inline)) {
            const uint32_t e = mw[rf >> 1] >> ((rf & 1) * 16 + 4 * gq);  // rows 16 rf + 4 g + j: bit j
#pragma unroll
            for (int qt = 0; qt < QS_QT; ++qt) acc[rf][qt] = mask_ineligible4(acc[rf][qt], e);
        };
        if constexpr (ABL & 8) {  // diagnostics: no epilogue (accumulators kept live)
#pragma unroll
            for (int rf = 0; rf < RF; ++rf)
#pragma unroll
                for (int qt = 0; qt < QS_QT; ++qt) asm volatile("" ::"v"(acc[rf][qt]));
            continue;
        }
        if constexpr (METRIC) {  // u >= thr[q] (the metric epilogue's comment in filter_mfma.h)
            // in place: the accumulators become u, and the test below (its maximum as the wave-uniform
            // early-out, then per row) is the cosine epilogue's own code on them.  Nothing of this
            // moves up among the tile's last MFMAs, where the row fragments are still live.
            __builtin_amdgcn_sched_barrier(0);
            const int64_t tile_row = a.r_begin + (rt0 + tile) * QS_RT;  // wave-uniform
            // (PAGED: the norms sit beside the rows, at the tile's local row; `left` stays in positions)
            const float *tn = fm.norms + (PAGED ? (int64_t)pg_epi * RC_PAGE_ROWS + (tile_row & (RC_PAGE_ROWS - 1)) : tile_row);
            const int left = (int)min<int64_t>(a.r_end - tile_row, (int64_t)QS_RT);
#pragma unroll
            for (int qt = 0; qt < QS_QT; ++qt) thr[qt] = a.thr[q0 + qt * 16 + lq];
            f32x4_t k4[QS_QT];
#pragma unroll
            for (int qt = 0; qt < QS_QT; ++qt) k4[qt] = *reinterpret_cast<const f32x4_t *>(fm.mcoef + 4 * (q0 + qt * 16) + 4 * lq);
#pragma unroll
            for (int rf = 0; rf < RF; ++rf) {
                const f32x4_t nv = load_norms4(tn, 4 * gq + rf * 16, left);
#pragma unroll
                for (int qt = 0; qt < QS_QT; ++qt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[rf][qt][j] = metric_upper(k4[qt], acc[rf][qt][j], nv[j]);
                if constexpr (MASKED) mask_rows(rf);  // here, under the same barriers: the NKT 8 form has no register for more
                if (rf % 4 == 3) __builtin_amdgcn_sched_barrier(0);  // at most four norm loads (16 registers) in flight
            }
        }
        if constexpr (MASKED && !METRIC) {
#pragma unroll
            for (int rf = 0; rf < RF; ++rf) mask_rows(rf);
        }
#pragma unroll
        for (int qt = 0; qt < QS_QT; ++qt) {
            const float th = thr[qt];
            float m = -INFINITY;
#pragma unroll
            for (int rf = 0; rf < RF; ++rf) {
                const f32x4_t v = acc[rf][qt];
                m = fmaxf(m, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
            }
            if (__ballot(m >= th) == 0) continue;  // wave-uniform: the common case
            if (m >= th) {
                const int q = q0 + qt * 16 + lq;
#pragma unroll
                for (int rf = 0; rf < RF; ++rf)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int64_t row = rbase + rf * 16 + j;
                        if (acc[rf][qt][j] >= th && row < a.r_end) append_candidate(a, q, row);
                    }
            }
        }
    }
}

// One filter dispatch of run_stages over local rows (PAGED: positions) [c0, c1) in nchunk row chunks.
// The kernel by row width (ld 128 / 256 / 512: query-stationary; every other: the generic GEMM), its
// METRIC form under a non-cosine metric, its MASKED form with BatchPlan::mask_filter.
// Not instantiated: the PAGED METRIC MASKED form at ld 512.  Its contiguous form sits at 256 VGPRs
// with nothing to spare, and with the page words it needs 8 bytes of scratch
// (tools/kernel_resources.py), also when the epilogue's page is loaded in the epilogue itself.
// paged_filter_supported says so to the callers.
template <typename T, bool PAGED>
void launch_filter_native(const BatchPlan &p, const BatchWs &ws, int64_t c0, int64_t c1, int64_t nchunk, int nqb, hipStream_t s) {
    const int nkt = (int)(p.ld / 64);
    const bool qs = nkt == 2 || nkt == 4 || nkt == 8;
    const FilterNativeArgs fa{FilterArgs{p.rows, ws.qh.get(), p.ld, nkt, c0, c1, tiles_per_chunk(c0, c1, qs ? QS_RT : SB_TILE, nchunk), nqb,
                                         ws.thr.get(), ws.cnt.get(), ws.cand.get(), ws.cap},
                              FilterMetric{p.norms, ws.mcoef.get()}, p.mask, p.pages};
    const dim3 gr((unsigned)(nchunk * nqb)), bl(512);
    auto launch = [&](auto metric, auto masked) {
        constexpr bool ME = decltype(metric)::value, MA = decltype(masked)::value;
        if (nkt == 8) {
            if constexpr (PAGED && ME && MA) throw Error(RC_ERR_UNSUPPORTED, "no paged metric filter with the mask inside at ld 512");
            else hipLaunchKernelGGL((filter_qs_kernel<T, 8, 0, ME, MA, PAGED>), gr, bl, 0, s, fa);
        } else if (nkt == 4) hipLaunchKernelGGL((filter_qs_kernel<T, 4, 0, ME, MA, PAGED>), gr, bl, 0, s, fa);
        else if (nkt == 2) hipLaunchKernelGGL((filter_qs_kernel<T, 2, 0, ME, MA, PAGED>), gr, bl, 0, s, fa);
        else hipLaunchKernelGGL((filter_gemm_kernel<T, ME, MA, PAGED>), gr, bl, 0, s, fa);
    };
    auto with_mask = [&](auto metric) {
        if (p.mask_filter) launch(metric, std::true_type{});
        else launch(metric, std::false_type{});
    };
    if (p.metric != RC_METRIC_COSINE) with_mask(std::true_type{});
    else with_mask(std::false_type{});
}
// the PAGED forms are search_mfma_paged.hip's
extern template void launch_filter_native<f16_t, true>(const BatchPlan &, const BatchWs &, int64_t, int64_t, int64_t, int, hipStream_t);
extern template void launch_filter_native<bf16_t, true>(const BatchPlan &, const BatchWs &, int64_t, int64_t, int64_t, int, hipStream_t);

}  // namespace rc
