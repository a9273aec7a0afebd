// filter_gemm_body.inc — the body of filter_gemm_kernel<T> and filter_gemm_metric_kernel<T>
// (search_mfma.hip), included inside each kernel's braces.  In scope: T, the kernel argument
// `FilterArgs a`, `constexpr bool METRIC` and (METRIC) `FilterMetric fm`, `constexpr bool MASKED` and
// (MASKED) `const uint32_t *mask` (filter_gemm_masked_kernel<T, METRIC>), `constexpr bool PAGED` and
// (PAGED) `const int32_t *pages` (filter_gemm_paged_kernel, search_mfma_paged.hip; filter_mfma.h,
// "PAGED forms").  Text inclusion, not a
// device function: as a function taking the arguments by reference the cosine kernel's registers
// and schedule change; this way it compiles to the instructions it had as the only copy.  (A
// `bool METRIC = false` template parameter on the kernel itself would read better, but the
// parameter is part of the kernel's mangled name: every cosine instantiation would be a new symbol,
// and tools/kernel_asm_diff.py, which pairs kernels by symbol, could no longer show them unchanged.)
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
                if constexpr (METRIC) {  // u >= thr[q] (the metric epilogue's comment in search_mfma.hip)
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
