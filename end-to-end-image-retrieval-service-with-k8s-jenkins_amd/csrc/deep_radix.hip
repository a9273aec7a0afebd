// deep_radix.hip — the one-shot selection of the deep top-k (deep.h, deep_select_radix): a radix
// select over the 64-bit keys.  A handful of digit passes find the k-th smallest key T of a
// query's stream exactly, one pass appends every eligible key <= T to the query's k output slots,
// and one block per query sorts them there.  The number of launches follows the width of the
// keys, not k.  DESIGN.md, "Deep top-k", has the design and the argument for exactness.
//
// The key (topk.h) is (~order(score), row): the passes walk the score word in three digits
// (11, 11 and 10 bits) and then only the row bits the call's largest row can have set, in digits
// of at most 12 bits, so a block's histogram (<= 4096 bins x 4 B) lives in LDS.
//
// Per query and pass p, device memory holds a histogram and a state (the prefix fixed by the
// digits above pass p, the rank still to be found inside it, a done flag).  Pass p's blocks each
// resolve pass p - 1's finished histogram in their prologue (a block-wide prefix scan over the
// bins; every block computes the same state, block 0 stores it for the record), so nothing but
// kernel boundaries orders the passes: no resolve launch, no ticket, no spin.
#include "deep.h"

namespace rc {

namespace {

constexpr int RADIX_THREADS = 256;
constexpr int SORT_THREADS = 1024;

// pass p counts digit (key >> shift[p]) & (2^bits[p] - 1) of the keys whose bits above
// shift[p - 1] equal the prefix (p == 0: every key)
struct RadixPlan {
    int npass;
    int shift[DEEP_RADIX_PASSES];
    int bits[DEEP_RADIX_PASSES];
};

struct RadixState {
    uint64_t prefix;  // the digits fixed so far; done: the bound T itself
    uint32_t rank;    // the rank of the k-th key among the stream's keys under the prefix, from 1
    uint32_t done;    // T is known: the later passes have nothing to count
};

// The workspace of a call of nq queries, carved from DeepSel::radix (u32 words):
// hist [DEEP_RADIX_PASSES][nq][DEEP_RADIX_BINS], state [DEEP_RADIX_PASSES + 1][nq], count [nq].
struct RadixWs {
    uint32_t *hist;
    RadixState *state;
    uint32_t *count;
};
__host__ __device__ inline RadixWs radix_ws(uint32_t *base, int nq) {
    RadixWs w;
    w.hist = base;
    w.state = (RadixState *)(base + (size_t)DEEP_RADIX_PASSES * nq * DEEP_RADIX_BINS);
    w.count = (uint32_t *)(w.state + (size_t)(DEEP_RADIX_PASSES + 1) * nq);
    return w;
}
constexpr size_t radix_ws_words(int nq) {
    return (size_t)DEEP_RADIX_PASSES * nq * DEEP_RADIX_BINS + (size_t)(DEEP_RADIX_PASSES + 1) * nq * (sizeof(RadixState) / 4) + nq;
}

// The start of a call: the histograms of its passes and the candidate counts cleared, state 0 =
// (no prefix, rank k).  A kernel, not a memset, so the call is the same in a captured stream.
__global__ __launch_bounds__(256) void radix_init_kernel(uint32_t *base, int nq, int npass, int k) {
    const RadixWs w = radix_ws(base, nq);
    const int64_t nh = (int64_t)npass * nq * DEEP_RADIX_BINS;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nh; i += (int64_t)gridDim.x * 256) w.hist[i] = 0u;
    if (blockIdx.x == 0) {
        for (int q = threadIdx.x; q < nq; q += 256) {
            w.count[q] = 0u;
            w.state[q] = RadixState{0ull, (uint32_t)k, 0u};
        }
    }
}

// Entry i of query q's stream: its key, and whether it is eligible (deep.h, DeepStream; exactly
// select_after_kernel's rule).  i < st.n.
template <bool KEYS>
__device__ __forceinline__ bool stream_entry(const DeepStream &st, const float *__restrict__ sc, int q, int64_t i, uint64_t &key) {
    if constexpr (KEYS) {
        const int64_t l = i / st.klist, t = i - l * st.klist;
        key = st.keys[(l * st.nq_total + st.q0 + q) * st.klist + t];
        return key != KEY_EMPTY;
    } else {
        key = make_key(sc[i], (uint32_t)(st.row_base + i * st.row_stride));
        return st.mask == nullptr || ((st.mask[i >> 5] >> (uint32_t)(i & 31)) & 1u) != 0u;
    }
}

// The state before pass p (p == npass: before the compaction) of query q, by every thread of a
// 256-thread block: pass p - 1's state advanced by its finished histogram.  The bin that holds
// the rank-th key is found by a block-wide prefix scan: the histogram is copied to `bins` (LDS,
// DEEP_RADIX_BINS words, overwritten), each thread sums 2^bits / 256 consecutive bins, a wave scan
// and the four wave totals place the thread's share, and the one thread whose share straddles the
// rank walks its bins.  Fewer keys than the rank (pass 0 only: fewer than k are eligible): T
// admits everything.  The bin holds exactly the keys still wanted: T = the bin's largest key, done.
__device__ RadixState radix_resolve(const RadixWs &w, const RadixPlan &plan, int nq, int q, int p, uint32_t *bins, uint32_t *wsum,
                                    RadixState *res) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RadixState prev = w.state[(size_t)(p - 1) * nq + q];
    if (prev.done) return prev;  // block-uniform
    const int nb = 1 << plan.bits[p - 1], shift = plan.shift[p - 1];
    const uint32_t *__restrict__ h = w.hist + ((size_t)(p - 1) * nq + q) * DEEP_RADIX_BINS;
    for (int i = tid; i < nb; i += RADIX_THREADS) bins[i] = h[i];
    __syncthreads();
    const int per = (nb + RADIX_THREADS - 1) / RADIX_THREADS;
    const int b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
    uint32_t mine = 0;
    for (int b = b0; b < b1; ++b) mine += bins[b];
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine, total = 0;
#pragma unroll
    for (int v = 0; v < RADIX_THREADS / 64; ++v) {
        if (v < wave) before += wsum[v];
        total += wsum[v];
    }
    if (total < prev.rank) {
        if (tid == 0) *res = RadixState{KEY_EMPTY, 0u, 1u};
    } else if (before < prev.rank && prev.rank <= before + mine) {  // one thread: the shares are disjoint
        uint32_t acc = before;
        int b = b0;
        while (acc + bins[b] < prev.rank) acc += bins[b++];  // ends inside [b0, b1): acc + the share >= rank
        RadixState r;
        r.prefix = prev.prefix | ((uint64_t)b << shift);
        r.rank = prev.rank - acc;
        r.done = bins[b] == r.rank ? 1u : 0u;
        if (r.done) r.prefix |= (1ull << shift) - 1ull;
        *res = r;
    }
    __syncthreads();
    const RadixState r = *res;
    __syncthreads();  // bins, wsum and res are free again
    return r;
}

// One digit pass.  Block (b, q) owns entries [b * per_block, ...) of query q's stream, as the
// rounds' blocks do: every wave reads its entries with coalesced loads, forms the key, tests the
// bitmap, keeps the entries whose higher digits equal the prefix and counts their digit into the
// LDS histogram; the block then adds its non-zero bins to the query's histogram of this pass.
template <bool KEYS>
__global__ __launch_bounds__(RADIX_THREADS) void radix_pass_kernel(const DeepStream st, int64_t per_block, int nq, int p,
                                                                   const RadixPlan plan, uint32_t *base) {
    __shared__ uint32_t bins[DEEP_RADIX_BINS];
    __shared__ uint32_t wsum[RADIX_THREADS / 64];
    __shared__ RadixState res;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y;
    const RadixWs w = radix_ws(base, nq);
    RadixState cur = w.state[q];
    if (p > 0) {
        cur = radix_resolve(w, plan, nq, q, p, bins, wsum, &res);
        if (blockIdx.x == 0 && tid == 0) w.state[(size_t)p * nq + q] = cur;
    }
    if (cur.done) return;  // block-uniform: an earlier digit settled T
    const int nb = 1 << plan.bits[p], shift = plan.shift[p];
    const int hs = p > 0 ? plan.shift[p - 1] : 0;  // the prefix covers the bits from hs up
    const uint64_t want = p > 0 ? cur.prefix >> hs : 0ull;
    for (int i = tid; i < nb; i += RADIX_THREADS) bins[i] = 0u;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * per_block;
    const int64_t i1 = min(st.n, i0 + per_block);
    const float *__restrict__ sc = KEYS ? nullptr : st.scores + (int64_t)q * st.n;
    constexpr int U = 4;  // independent loads in flight per lane before any is consumed
    for (int64_t j0 = i0 + (int64_t)wave * 64 * U; j0 < i1; j0 += RADIX_THREADS * U) {
        uint64_t key[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = j0 + u * 64 + lane;
            key[u] = KEY_EMPTY;
            ok[u] = i < i1 && stream_entry<KEYS>(st, sc, q, i, key[u]);  // i < st.n: inside the scores, the lists and the bitmap
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (ok[u] && (p == 0 || (key[u] >> hs) == want)) atomicAdd(&bins[(uint32_t)(key[u] >> shift) & (uint32_t)(nb - 1)], 1u);
        }
    }
    __syncthreads();
    uint32_t *__restrict__ h = w.hist + ((size_t)p * nq + q) * DEEP_RADIX_BINS;
    for (int i = tid; i < nb; i += RADIX_THREADS) {
        const uint32_t c = bins[i];
        if (c != 0u) atomicAdd(&h[i], c);
    }
}

// The compaction: the last pass's histogram resolved to T, then one pass over the stream that
// appends every eligible key <= T to out_keys[q * k ..), one atomic per wave (ballot, popcount,
// lane-prefix offset).  The keys are distinct, so exactly min(k, eligible) arrive; the guard on
// the slot only keeps a caller's duplicate keys from writing past the query's k slots.
template <bool KEYS>
__global__ __launch_bounds__(RADIX_THREADS) void radix_compact_kernel(const DeepStream st, int64_t per_block, int nq, int k,
                                                                      const RadixPlan plan, uint32_t *base, uint64_t *__restrict__ out_keys) {
    __shared__ uint32_t bins[DEEP_RADIX_BINS];
    __shared__ uint32_t wsum[RADIX_THREADS / 64];
    __shared__ RadixState res;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y;
    const RadixWs w = radix_ws(base, nq);
    const RadixState cur = radix_resolve(w, plan, nq, q, plan.npass, bins, wsum, &res);
    const uint64_t T = cur.prefix;
    uint64_t *__restrict__ dst = out_keys + (int64_t)q * k;
    const int64_t i0 = (int64_t)blockIdx.x * per_block;
    const int64_t i1 = min(st.n, i0 + per_block);
    const float *__restrict__ sc = KEYS ? nullptr : st.scores + (int64_t)q * st.n;
    constexpr int U = 4;
    for (int64_t j0 = i0 + (int64_t)wave * 64 * U; j0 < i1; j0 += RADIX_THREADS * U) {
        uint64_t key[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = j0 + u * 64 + lane;
            key[u] = KEY_EMPTY;
            ok[u] = i < i1 && stream_entry<KEYS>(st, sc, q, i, key[u]) && key[u] <= T;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t votes = __ballot(ok[u]);
            if (votes == 0ull) continue;  // wave-uniform
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(&w.count[q], (uint32_t)__popcll(votes));
            at = __shfl(at, 0) + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
            if (ok[u] && at < (uint32_t)k) dst[at] = key[u];
        }
    }
}

// The sort: one block per query.  The query's candidates, padded with KEY_EMPTY to N (a power of
// two >= k), are sorted ascending in LDS by a bitonic network and the first k written back to
// out_keys[q * k ..), where the compaction left them.
template <int N>
__global__ __launch_bounds__(SORT_THREADS) void radix_sort_kernel(int nq, int k, uint32_t *base, uint64_t *__restrict__ out_keys) {
    __shared__ uint64_t v[N];
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const int have = (int)min(radix_ws(base, nq).count[q], (uint32_t)k);
    uint64_t *__restrict__ dst = out_keys + (int64_t)q * k;
    for (int i = tid; i < N; i += SORT_THREADS) v[i] = i < have ? dst[i] : KEY_EMPTY;
    __syncthreads();
    for (int kk = 2; kk <= N; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < N / 2; t += SORT_THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint64_t a = v[lo], b = v[hi];
                if ((a > b) == ((lo & kk) == 0)) {
                    v[lo] = b;
                    v[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += SORT_THREADS) dst[i] = v[i];
}

__global__ __launch_bounds__(256) void radix_fill_empty_kernel(uint64_t *__restrict__ keys, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = KEY_EMPTY;
}

// Three digits over the score word, then the row bits up to the largest row's highest set bit in
// as few digits of at most 12 bits as cover them, split evenly.
RadixPlan make_plan(uint32_t row_max) {
    RadixPlan plan{};
    int np = 0;
    const int score_bits[3] = {11, 11, 10};
    int at = 64;
    for (int b : score_bits) {
        at -= b;
        plan.shift[np] = at;
        plan.bits[np++] = b;
    }
    int row_bits = 0;
    while (row_bits < 32 && (row_max >> row_bits) != 0u) ++row_bits;
    const int nrow = (row_bits + 11) / 12;
    at = row_bits;
    for (int i = 0; i < nrow; ++i) {
        const int b = (at + (nrow - i) - 1) / (nrow - i);
        at -= b;
        plan.shift[np] = at;
        plan.bits[np++] = b;
    }
    plan.npass = np;
    return plan;
}

template <int N>
void launch_sort(int nq, int k, uint32_t *base, uint64_t *out_keys, hipStream_t s) {
    hipLaunchKernelGGL(radix_sort_kernel<N>, dim3(nq), dim3(SORT_THREADS), 0, s, nq, k, base, out_keys);
}

}  // namespace

void DeepSel::ensure_radix(int nq) {
    radix.reserve(radix_ws_words(nq));  // grows with nq
}

void deep_select_radix(const DeepStream &st, DeepSel &ws, int nq, int k, uint64_t *out_keys, hipStream_t s) {
    if (nq <= 0 || k <= 0) return;
    if (nq > ws.nq_cap || st.n < 0 || (st.scores == nullptr) == (st.keys == nullptr) || k > DEEP_RADIX_SORT_MAX)
        throw Error(RC_ERR_INVALID, "internal: deep selection over an unprepared workspace or stream");
    if (st.n == 0) {  // nothing to select from: every slot is empty
        const int64_t n = (int64_t)nq * k;
        hipLaunchKernelGGL(radix_fill_empty_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out_keys, n);
        RC_LAUNCH_CHECK();
        return;
    }
    ws.ensure_radix(nq);
    // the largest row a key of this call can carry: the scores form's own last entry; ready keys
    // say nothing of their rows, so the leader's few lists are walked over every row bit
    const int64_t last = st.scores != nullptr ? st.row_base + (st.n - 1) * st.row_stride : -1;
    const RadixPlan plan = make_plan(last < 0 || last > 0xffffffffll ? 0xffffffffu : (uint32_t)last);
    // the rounds' split: a block owns at least RC_DEEP_SELECT_ROWS entries, at most DEEP_SELECT_BLOCKS blocks
    int nblk = (int)std::min<int64_t>(DEEP_SELECT_BLOCKS, (st.n + RC_DEEP_SELECT_ROWS - 1) / RC_DEEP_SELECT_ROWS);
    int64_t per_block = (st.n + nblk - 1) / nblk;
    per_block = (per_block + 31) / 32 * 32;
    nblk = (int)((st.n + per_block - 1) / per_block);
    const bool lists = st.keys != nullptr;
    const int64_t nh = (int64_t)plan.npass * nq * DEEP_RADIX_BINS;
    hipLaunchKernelGGL(radix_init_kernel, dim3((unsigned)std::min<int64_t>(1024, (nh + 255) / 256)), dim3(256), 0, s, ws.radix.get(), nq,
                       plan.npass, k);
    RC_LAUNCH_CHECK();
    for (int p = 0; p < plan.npass; ++p) {
        if (lists) hipLaunchKernelGGL(radix_pass_kernel<true>, dim3(nblk, nq), dim3(RADIX_THREADS), 0, s, st, per_block, nq, p, plan, ws.radix.get());
        else hipLaunchKernelGGL(radix_pass_kernel<false>, dim3(nblk, nq), dim3(RADIX_THREADS), 0, s, st, per_block, nq, p, plan, ws.radix.get());
        RC_LAUNCH_CHECK();
    }
    if (lists)
        hipLaunchKernelGGL(radix_compact_kernel<true>, dim3(nblk, nq), dim3(RADIX_THREADS), 0, s, st, per_block, nq, k, plan, ws.radix.get(), out_keys);
    else
        hipLaunchKernelGGL(radix_compact_kernel<false>, dim3(nblk, nq), dim3(RADIX_THREADS), 0, s, st, per_block, nq, k, plan, ws.radix.get(), out_keys);
    RC_LAUNCH_CHECK();
    // the LDS the sort asks for follows k: 4 KB to 128 KB
    if (k <= 512) launch_sort<512>(nq, k, ws.radix.get(), out_keys, s);
    else if (k <= 2048) launch_sort<2048>(nq, k, ws.radix.get(), out_keys, s);
    else if (k <= 8192) launch_sort<8192>(nq, k, ws.radix.get(), out_keys, s);
    else launch_sort<DEEP_RADIX_SORT_MAX>(nq, k, ws.radix.get(), out_keys, s);
    RC_LAUNCH_CHECK();
}

}  // namespace rc
