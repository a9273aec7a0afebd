// filter_qs_body.inc — the body of filter_qs_kernel<T, NKT, ABL> and filter_qs_metric_kernel<T, NKT>
// (search_mfma.hip), included inside each kernel's braces.  In scope: T, NKT, ABL, the kernel
// argument `FilterArgs a`, `constexpr bool METRIC` and (METRIC) `FilterMetric fm`, `constexpr bool
// MASKED` and (MASKED) `const uint32_t *mask` (filter_qs_masked_kernel<T, NKT, METRIC>), `constexpr
// bool PAGED` and (PAGED) `const int32_t *pages` (filter_qs_paged_kernel, search_mfma_paged.hip;
// filter_mfma.h, "PAGED forms").  Text inclusion, not a device function, for the reason given in
// filter_gemm_body.inc.
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
        if constexpr (METRIC) {  // u >= thr[q] (the metric epilogue's comment in search_mfma.hip)
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
