// deep_select.hip — the selection stage of the deep top-k (deep.h): a bounded top-RC_TOPK_MAX over
// a key stream, chained over ceil(k / RC_TOPK_MAX) rounds without the host.
//
// The key (topk.h) is a total order: ascending key = score descending, then row ascending, and no
// two entries of a stream share a key (each carries its own row).  The k smallest keys in order
// are therefore the RC_TOPK_MAX smallest, then the RC_TOPK_MAX smallest of the keys strictly
// greater than the last of those, and so on: round j selects among the keys >= lower, and the
// step that finishes it stores lower = its last key + 1 for round j + 1 (KEY_EMPTY once a round
// came up short: nothing is left, every later round admits nothing).  A tie in score that spans a
// round boundary is split by row, exactly where one sorted list of k keys would split it.
#include "deep.h"

namespace rc {

// One round's block pass.  Block (b, q) owns entries [b * per_block, ...) of query q's stream; each
// wave keeps the k smallest admitted keys of its share (WaveTopK<512>, k <= RC_TOPK_MAX), wave 0
// folds the four lists and writes partial list (b, q): k sorted keys, KEY_EMPTY-padded.
// A candidate is admitted iff key >= lower[q] (read once, at kernel start) and it is eligible:
// its mask bit (scores form, mask given) or key != KEY_EMPTY (keys form).
template <bool KEYS>
__global__ __launch_bounds__(256) void select_after_kernel(const DeepStream st, int64_t per_block, int nq, int k,
                                                          const uint64_t *__restrict__ lower, uint64_t *__restrict__ partial) {
    __shared__ uint64_t lds[4][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.y;
    uint64_t *dst = partial + ((int64_t)blockIdx.x * nq + q) * k;
    const uint64_t lo = lower[q];
    if (lo == KEY_EMPTY) {  // block-uniform: an earlier round came up short
        for (int j = threadIdx.x; j < k; j += 256) dst[j] = KEY_EMPTY;
        return;
    }
    WaveTopK<512> tk;
    tk.init(as_lds(&lds[wave][0]), k);
    const int64_t i0 = (int64_t)blockIdx.x * per_block;
    const int64_t i1 = min(st.n, i0 + per_block);
    const float *__restrict__ sc = KEYS ? nullptr : st.scores + (int64_t)q * st.n;
    constexpr int U = 4;  // independent loads in flight per lane before any is consumed
    for (int64_t j0 = i0 + (int64_t)wave * 64 * U; j0 < i1; j0 += 256 * U) {
        uint64_t key[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = j0 + u * 64 + lane;
            key[u] = KEY_EMPTY;
            ok[u] = false;
            if (i < i1) {  // i < st.n: inside the scores, the lists and the bitmap's ceil(n / 32) words
                if constexpr (KEYS) {
                    const int64_t l = i / st.klist, t = i - l * st.klist;
                    key[u] = st.keys[(l * st.nq_total + st.q0 + q) * st.klist + t];
                    ok[u] = key[u] != KEY_EMPTY;
                } else {
                    key[u] = make_key(sc[i], (uint32_t)(st.row_base + i * st.row_stride));
                    ok[u] = st.mask == nullptr || ((st.mask[i >> 5] >> (uint32_t)(i & 31)) & 1u) != 0u;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            tk.reserve(64);
            tk.push(ok[u] && key[u] >= lo, key[u]);
        }
    }
    tk.compact();
    __syncthreads();
    if (wave == 0) {
        RC_FOLD_WAVE_LISTS(&lds[w][0], tk, k, lane);
        for (int j = lane; j < k; j += 64) dst[j] = tk.buf[j];
    }
}

// The step that finishes a round: one block per query merges the blocks' partial lists (the
// existing merge), writes the round's k sorted keys to out_keys[q * kout + off ..) and leaves the
// next round's bound.  The bound is an ordinary store from lane 0 of wave 0; the kernel boundary
// orders it before the next round's reads.
__global__ __launch_bounds__(256) void select_finish_kernel(const uint64_t *__restrict__ partial, int nlist, int nq, int k,
                                                           uint64_t *__restrict__ lower, uint64_t *__restrict__ out_keys,
                                                           int64_t kout, int64_t off) {
    __shared__ uint64_t lds[4][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x;
    uint64_t *dst = out_keys + (int64_t)q * kout + off;
    if (lower[q] == KEY_EMPTY) {  // block-uniform: every list of this round is empty
        for (int j = threadIdx.x; j < k; j += 256) dst[j] = KEY_EMPTY;
        return;
    }
    WaveTopK<512> tk;
    merge_partial_lists<512>(partial, nlist, nq, q, k, lds, tk);
    if (wave == 0) {
        for (int j = lane; j < k; j += 64) dst[j] = tk.buf[j];
        if (lane == 0) {
            const uint64_t last = tk.buf[k - 1];
            lower[q] = last == KEY_EMPTY ? KEY_EMPTY : last + 1;  // a real key's row word is below 2^32 - 1
        }
    }
}

__global__ __launch_bounds__(256) void deep_emit_kernel(const uint64_t *__restrict__ keys, int64_t n, float *__restrict__ scores,
                                                       int64_t *__restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    RC_EMIT_KEY(key, 0, 1, scores[i], rows[i]);
}

void DeepSel::ensure(int nq, int64_t nkeys) {
    if (nq > nq_cap) {
        dfree(partial);
        dfree(lower);
        partial = lower = nullptr;
        nq_cap = 0;
        partial = (uint64_t *)dmalloc((size_t)DEEP_SELECT_BLOCKS * nq * RC_TOPK_MAX * sizeof(uint64_t));
        lower = (uint64_t *)dmalloc((size_t)nq * sizeof(uint64_t));
        nq_cap = nq;
    }
    if (nkeys > keys_cap) {
        dfree(keys);
        keys = nullptr;
        keys_cap = 0;
        keys = (uint64_t *)dmalloc((size_t)nkeys * sizeof(uint64_t));
        keys_cap = nkeys;
    }
}

void DeepSel::release() {
    dfree(partial);
    dfree(lower);
    dfree(keys);
    partial = lower = keys = nullptr;
    nq_cap = 0;
    keys_cap = 0;
}

void deep_select_rounds(const DeepStream &st, DeepSel &ws, int nq, int k, uint64_t *out_keys, hipStream_t s) {
    if (nq <= 0 || k <= 0) return;
    if (nq > ws.nq_cap || st.n < 0 || (st.scores == nullptr) == (st.keys == nullptr))
        throw Error(RC_ERR_INVALID, "internal: deep selection over an unprepared workspace or stream");
    if (st.n == 0) {  // nothing to select from: every slot is empty
        RC_HIP(hipMemsetAsync(out_keys, 0xff, (size_t)nq * k * sizeof(uint64_t), s));
        return;
    }
    // a block owns at least RC_DEEP_SELECT_ROWS entries, and there are at most DEEP_SELECT_BLOCKS lists
    int nblk = (int)std::min<int64_t>(DEEP_SELECT_BLOCKS, (st.n + RC_DEEP_SELECT_ROWS - 1) / RC_DEEP_SELECT_ROWS);
    int64_t per_block = (st.n + nblk - 1) / nblk;
    per_block = (per_block + 31) / 32 * 32;
    nblk = (int)((st.n + per_block - 1) / per_block);
    RC_HIP(hipMemsetAsync(ws.lower, 0, (size_t)nq * sizeof(uint64_t), s));  // round 0 admits every key
    for (int off = 0; off < k; off += RC_TOPK_MAX) {
        const int kr = std::min(RC_TOPK_MAX, k - off);
        if (st.keys != nullptr)
            hipLaunchKernelGGL(select_after_kernel<true>, dim3(nblk, nq), dim3(256), 0, s, st, per_block, nq, kr, ws.lower, ws.partial);
        else
            hipLaunchKernelGGL(select_after_kernel<false>, dim3(nblk, nq), dim3(256), 0, s, st, per_block, nq, kr, ws.lower, ws.partial);
        RC_LAUNCH_CHECK();
        hipLaunchKernelGGL(select_finish_kernel, dim3(nq), dim3(256), 0, s, ws.partial, nblk, nq, kr, ws.lower, out_keys, (int64_t)k,
                           (int64_t)off);
        RC_LAUNCH_CHECK();
    }
}

void deep_emit(const uint64_t *keys, int64_t n, float *scores, int64_t *rows, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(deep_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, keys, n, scores, rows);
    RC_LAUNCH_CHECK();
}

}  // namespace rc
