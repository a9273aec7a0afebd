// rescore_body.inc — the body of rescore_kernel and rescore_metric_kernel (rescore.h), included
// inside each kernel's braces.  In scope: T, NCH, CAP, MASKED, the kernels' arguments (each kernel
// declares the ones only the other takes as null constants), `constexpr bool METRIC`, and
// `constexpr bool PAGED` with (PAGED) `const int32_t *pages` (rescore_paged_kernel: the candidates,
// the mask bits and the keys are POSITIONS of a page table, and only the row and norm address goes
// through it, as scan_paged.h's scan).  Text inclusion, not a device function: the cosine kernels
// keep the instructions they had.
    constexpr int EPC = RowShape<T, NCH>::EPC;
    constexpr int CPL = RowShape<T, NCH>::CPL;
    constexpr int U = 2;
    __shared__ uint64_t lds[4][CAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rg = lane >> 4;
    const int qi = blockIdx.x;

    float q[1][CPL][EPC];
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            q[0][i][e] = qn[(int64_t)qi * ld + (sub + 16 * i) * EPC + e];
            if constexpr (sizeof(T) == 1) q[0][i][e] *= query_unscale<T>();  // as scan_rows: the scan's bits
        }

    [[maybe_unused]] MetricCoef mc{};
    if constexpr (METRIC) mc = MetricCoef{mcoef[4 * qi + 1], mcoef[4 * qi + 2], mcoef[4 * qi + 3]};  // block-uniform

    const uint32_t n = cnt[qi];
    const int nn = (int)min<uint32_t>(n, (uint32_t)cap);
    const uint32_t *cl = cand + (int64_t)qi * cap;
    const uint4 *base4 = reinterpret_cast<const uint4 *>(rows);
    const int64_t ld4 = ld / EPC;

    WaveTopK<CAP> tk;
    tk.init(as_lds(&lds[wave][0]), k);
    if (wave == 0) {  // the running top-k of the earlier stages
        for (int j = 0; j < k; j += 64) {
            const uint64_t key = (j + lane < k) ? keys[(int64_t)qi * k + j + lane] : KEY_EMPTY;
            tk.reserve(64);
            tk.push(key != KEY_EMPTY, key);
        }
    }
    for (int j0 = wave * 4 * U; j0 < nn; j0 += 16 * U) {
        uint4 x[U][CPL];
        uint32_t rr[U];
        [[maybe_unused]] uint32_t lr[U];  // PAGED: the local row of position rr[u]
        [[maybe_unused]] uint32_t mw[U];
        [[maybe_unused]] float nrm[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * 4 + rg;
            rr[u] = cl[j < nn ? j : 0];
            if constexpr (MASKED) mw[u] = mask[rr[u] >> 5];
            if constexpr (PAGED) {  // a candidate position is < r_end <= n_pos: inside the table
                lr[u] = (uint32_t)pages[rr[u] / RC_PAGE_ROWS] * RC_PAGE_ROWS + rr[u] % RC_PAGE_ROWS;
                if constexpr (METRIC) nrm[u] = norms[lr[u]];
#pragma unroll
                for (int i = 0; i < CPL; ++i) x[u][i] = base4[(int64_t)lr[u] * ld4 + sub + 16 * i];
                continue;
            }
            if constexpr (METRIC) nrm[u] = norms[rr[u]];  // a candidate row is < r_end <= n_rows
#pragma unroll
            for (int i = 0; i < CPL; ++i) x[u][i] = base4[(int64_t)rr[u] * ld4 + sub + 16 * i];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * 4 + rg;
            float acc[1];
            RC_ROW_FMA16(T, 1, CPL, EPC, x[u], q, acc);
            float s = sum16(acc[0]);
            if constexpr (METRIC) s = metric_score(mc, s, nrm[u]);
            tk.reserve(4);
            if constexpr (MASKED) tk.push(sub == 0 && j < nn && ((mw[u] >> (rr[u] & 31u)) & 1u) != 0u, make_key(s, rr[u]));
            else tk.push(sub == 0 && j < nn, make_key(s, rr[u]));
        }
    }
    tk.compact();
    __syncthreads();
    if (wave == 0) {
        RC_FOLD_WAVE_LISTS(&lds[w][0], tk, k, lane);
        for (int j = lane; j < k; j += 64) {
            const uint64_t key = tk.buf[j];
            keys[(int64_t)qi * k + j] = key;
            if (final_pass) {
                RC_EMIT_KEY(key, row_base, row_stride, out_scores[(int64_t)qi * k + j], out_rows[(int64_t)qi * k + j]);
            }
        }
        if (lane == 0) {
            if constexpr (METRIC) thr[qi] = tk.count >= k ? key_score(tk.buf[k - 1]) : -INFINITY;
            else thr[qi] = tk.count >= k ? key_score(tk.buf[k - 1]) - eps[qi] : -INFINITY;
            if (n > (uint32_t)cap && flags[qi] == 0) {
                flags[qi] = 1;
                atomicAdd(ovf_total, 1);
            }
            cnt[qi] = 0;
        }
    }
