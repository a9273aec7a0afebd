// index.hip — the in-HBM exact cosine index that replaces Pinecone
// (reference: get_index ingesting/utils.py:23-38, upsert ingesting/main.py:156-158,
//  query retriever/utils.py:59-66, fetch retriever/main.py:142).
//
// HBM layout: rows [capacity][ld] in the storage dtype (f32 / f16 / bf16 / f8: e4m3 bytes of
// the direction x 2^8, index_common.h), L2-normalised at upsert, ld = 128 * nch (zero-padded;
// nch even for f8), plus norms [capacity] f32.
//
// Search (single / few queries) is one streaming pass over the rows:
//   scan_topk_kernel: 16 lanes per row, 16-B loads, f32 FMA against the
//     query held in registers, DPP reduction across the 16 lanes, then a
//     wavefront top-k (ballot-filtered append against a running threshold +
//     register bitonic sort) per wave, merged per block → partial keys;
//   merge_partials_kernel: per query, top-k over all blocks' partial lists.
// Algorithmic HBM bytes per query pass: n_rows * ld * sizeof(T).
// Under a non-cosine metric (rc_index_set_metric) the same pass runs the metric kernels
// (scan_metric.h): each row's key carries q · v_r or −‖q − v_r‖² instead of the cosine, formed
// from the cosine and norms[r] before the top-k; nothing after the push differs.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "deep.h"
#include "sparse.h"
#include "paged.h"

namespace rc {

static thread_local std::string g_last_error;
void set_last_error(const std::string &m) { g_last_error = m; }

// ------------------------------------------------------- upsert / fetch --
// One wave per vector: norm in f32, normalise, cast, scatter to its row slot.
// src (optional): vector v is read from vecs[src[v]] (a shard's subset of a batch).
template <typename T>
__global__ __launch_bounds__(256) void upsert_kernel(T *__restrict__ rows, float *__restrict__ norms, int64_t ld, int dim,
                                                    const float *__restrict__ vecs, const int64_t *__restrict__ src_idx,
                                                    const int64_t *__restrict__ slot, int64_t n, int64_t cap) {
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= n) return;
    const int64_t r = slot[v];
    if (r < 0 || r >= cap) return;  // device-side guard: never write outside the row slots (hosts validate first)
    const float *src = vecs + (src_idx ? src_idx[v] : v) * dim;
    float ss = 0.f;
    for (int c = lane; c < dim; c += 64) ss = fmaf(src[c], src[c], ss);
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
    const float inv = nrm > 0.f ? 1.0f / nrm : 0.f;
    T *dst = rows + r * ld;
    for (int c = lane; c < ld; c += 64) dst[c] = Elem<T>::cast(c < dim ? src[c] * inv : 0.f);
    if (lane == 0) norms[r] = nrm;
}

template <typename T>
__global__ __launch_bounds__(256) void fetch_kernel(const T *__restrict__ rows, const float *__restrict__ norms, int64_t ld,
                                                   int dim, const int64_t *__restrict__ slot, int64_t n,
                                                   float *__restrict__ out, int64_t cap) {
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= n) return;
    const int64_t r = slot[v];
    if (r < 0 || r >= cap) {  // out of range: NaN values, never a read outside the rows
        for (int c = lane; c < dim; c += 64) out[v * dim + c] = __builtin_nanf("");
        return;
    }
    const float nrm = norms ? norms[r] : 1.0f;
    for (int c = lane; c < dim; c += 64) out[v * dim + c] = Elem<T>::load(rows, r * ld + c) * nrm;
}

// Row move (Index.delete's swap-remove compaction): stored row dst_idx[v] of the destination
// block = stored row src_idx[v] of the source block, bit for bit, with its f32 norm.  A null
// list means "contiguous from row 0 of that block", so the one kernel moves rows inside a
// shard (both lists, one block), packs a shard's outgoing rows into a staging block (source
// list only) and unpacks a staging block into a shard's rows (destination list only).  One wave
// per row, 16-byte pieces (ld is a multiple of 128 elements: a row is a whole number of them for
// every dtype), four loads in flight per lane; grid-stride over the rows.  An index outside its
// block is skipped, never read or written (the guard of upsert_kernel).  The int8 filter copy is
// not moved: the host re-quantises the destination slots (launch_move_rows).
// Callers keep the rows read and the rows written disjoint and every destination distinct.
template <typename T>
__global__ __launch_bounds__(256) void move_rows_kernel(const T *__restrict__ src_rows, const float *__restrict__ src_norms,
                                                       const int64_t *__restrict__ src_idx, int64_t src_cap,
                                                       T *__restrict__ dst_rows, float *__restrict__ dst_norms,
                                                       const int64_t *__restrict__ dst_idx, int64_t dst_cap, int64_t ld,
                                                       int64_t n) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    const int pieces = (int)(ld * (int64_t)sizeof(T) / 16);
    for (int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < n; v += nw) {
        const int64_t rs = src_idx ? src_idx[v] : v;
        const int64_t rd = dst_idx ? dst_idx[v] : v;
        if (rs < 0 || rs >= src_cap || rd < 0 || rd >= dst_cap) continue;  // wave-uniform
        const uint4 *sp = reinterpret_cast<const uint4 *>(src_rows + rs * ld);
        uint4 *dp = reinterpret_cast<uint4 *>(dst_rows + rd * ld);
        // a lane's pieces in groups of 4, then 2, then 1: inside a group nothing is predicated, so
        // its loads are all issued before the first store waits (with a bounds test per piece
        // hipcc sinks every load into its store's branch: one load in flight)
        int c = lane;
        for (; c + 192 < pieces; c += 256) {
            const uint4 t0 = sp[c], t1 = sp[c + 64], t2 = sp[c + 128], t3 = sp[c + 192];
            dp[c] = t0;
            dp[c + 64] = t1;
            dp[c + 128] = t2;
            dp[c + 192] = t3;
        }
        for (; c + 64 < pieces; c += 128) {
            const uint4 t0 = sp[c], t1 = sp[c + 64];
            dp[c] = t0;
            dp[c + 64] = t1;
        }
        if (c < pieces) dp[c] = sp[c];
        if (lane == 0) dst_norms[rd] = src_norms[rs];
    }
}

// splitmix64 finaliser: the synthetic-row generator (reproducible in numpy).
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ float synth_value(uint64_t seed, int64_t row, int dim, int c) {
    const uint64_t h = splitmix64(seed * 0xD1342543DE82EF95ull + (uint64_t)row * (uint64_t)dim + (uint64_t)c);
    return (float)(int32_t)(h >> 40) * (1.0f / 8388608.0f) - 1.0f;  // 24-bit uniform in [-1, 1)
}

template <typename T>
__global__ __launch_bounds__(256) void fill_random_kernel(T *__restrict__ rows, float *__restrict__ norms, int64_t ld,
                                                         int dim, uint64_t seed, int64_t row0, int64_t n) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < n; v += nw) {
        const int64_t r = row0 + v;
        float ss = 0.f;
        for (int c = lane; c < dim; c += 64) {
            const float x = synth_value(seed, r, dim, c);
            ss = fmaf(x, x, ss);
        }
        ss = wave_sum(ss);
        const float nrm = sqrtf(ss);
        const float inv = 1.0f / nrm;
        T *dst = rows + r * ld;
        for (int c = lane; c < ld; c += 64) dst[c] = Elem<T>::cast(c < dim ? synth_value(seed, r, dim, c) * inv : 0.f);
        if (lane == 0) norms[r] = nrm;
    }
}

// The int8 filter copy (search_mfma.hip, filter_i8_kernel): one wave per stored row x̂,
// sx = max|x̂| / 127, x8 = rne(x̂ / sx) clamped to [-127, 127], ex = ||x̂ - sx·x8||₂ rounded
// up (i8_scale / i8_round / i8_resid_bound, which the queries share), sx and ex at
// i8_slot(row).  Rows come from slots[v] (upsert) or row0 + v (fill / import / enable).
template <typename T>
__global__ __launch_bounds__(256) void quantize_rows_kernel(const T *__restrict__ rows, int64_t ld,
                                                           const int64_t *__restrict__ slots, int64_t row0, int64_t n,
                                                           int64_t cap, int8_t *__restrict__ rows8, float *__restrict__ rsx,
                                                           float *__restrict__ rex) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < n; v += nw) {
        const int64_t r = slots ? slots[v] : row0 + v;
        if (r < 0 || r >= cap) continue;  // wave-uniform
        const T *src = rows + r * ld;
        float mx = 0.f;
        for (int c = lane; c < ld; c += 64) mx = fmaxf(mx, fabsf(Elem<T>::load(src, c)));
        mx = wave_max(mx);
        const float s = i8_scale(mx), is = i8_inv_scale(mx);
        float e = 0.f;
        int8_t *dst = rows8 + r * ld;
        for (int c = lane; c < ld; c += 64) {
            const float x = Elem<T>::load(src, c);
            const float q = i8_round(x, is);
            dst[c] = (int8_t)q;
            const float d = x - s * q;
            e = fmaf(d, d, e);
        }
        e = wave_sum(e);
        if (lane == 0) {
            rsx[i8_slot(r)] = s;
            rex[i8_slot(r)] = i8_resid_bound(e);
        }
    }
}

// One block per query: top-k over nlist sorted partial lists of k keys each.
// flags (optional): only queries with flags[q] != 0 are merged (the batched
// search's exact fallback).  Returned row = row_base + local row * row_stride.
template <int CAP>
__global__ __launch_bounds__(256) void merge_partials_kernel(const uint64_t *__restrict__ partial, int nlist,
                                                            int nq_total, int k, int64_t row_base, int64_t row_stride,
                                                            const int *__restrict__ flags,
                                                            float *__restrict__ out_scores,
                                                            int64_t *__restrict__ out_rows) {
    __shared__ uint64_t lds[4][CAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = blockIdx.x;
    if (flags != nullptr && flags[qi] == 0) return;  // block-uniform
    WaveTopK<CAP> tk;
    merge_partial_lists<CAP>(partial, nlist, nq_total, qi, k, lds, tk);
    if (wave == 0) {
        for (int j = lane; j < k; j += 64) {
            const uint64_t key = tk.buf[j];
            RC_EMIT_KEY(key, row_base, row_stride, out_scores[(int64_t)qi * k + j], out_rows[(int64_t)qi * k + j]);
        }
    }
}

// Top-k of many sorted partial lists, one query per block (config 3: 1M rows = 1024 scan blocks,
// lists of k keys).  The answer's k-th key is at most hk, the k-th smallest of the lists' heads
// (k heads are <= hk), and a sorted list can only contribute its prefix <= hk: so the block takes
// the heads' top-k (one load per list, all in flight), then appends the prefixes <= hk of the
// lists whose head qualifies (usually about k keys in all), then sorts those.  The same keys as
// merging every list (merge_partial_lists, which loads all nlist·k keys: round 4's one block over
// ~2000 lists was 30.5 us, the two-level form after it 11 + 12 us); more than CAP candidates
// (adversarial inputs) fall back to that full merge inside the block.
constexpr int MERGE_HEADS_MIN = 64;  // fewer lists: merge_partials_kernel (all keys) is as fast
template <int CAP>
__global__ __launch_bounds__(256) void merge_heads_kernel(const uint64_t *__restrict__ partial, int nlist, int nq_total,
                                                         int k, int64_t row_base, int64_t row_stride,
                                                         const int *__restrict__ flags, float *__restrict__ out_scores,
                                                         int64_t *__restrict__ out_rows) {
    __shared__ uint64_t lds[4][CAP];
    __shared__ uint64_t cand[CAP];
    __shared__ uint64_t hk_s;
    __shared__ int ccount;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const int qi = blockIdx.x;
    if (flags != nullptr && flags[qi] == 0) return;  // block-uniform
    auto at = [&](int l, int t) { return partial[((int64_t)l * nq_total + qi) * k + t]; };
    WaveTopK<CAP> tk;
    tk.init(as_lds(&lds[wave][0]), k);
    // 1. the heads' top-k: HU heads per lane in flight, then per-wave top-k, then wave 0 over 4·k
    constexpr int HU = 8;
    for (int l0 = 0; l0 < nlist; l0 += 256 * HU) {
        uint64_t h[HU];
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            const int l = l0 + u * 256 + tid;
            h[u] = l < nlist ? at(l, 0) : KEY_EMPTY;
        }
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            tk.reserve(64);
            tk.push(h[u] != KEY_EMPTY, h[u]);
        }
    }
    tk.compact();
    if (tid == 0) ccount = 0;
    __syncthreads();
    if (wave == 0) {
        fold_wave_lists<CAP>(&lds[0][0], CAP, tk, k);
        if (lane == 0) hk_s = tk.count >= k ? tk.buf[k - 1] : KEY_EMPTY;
    }
    __syncthreads();
    const uint64_t hk = hk_s;
    // 2. the prefixes <= hk of the lists whose head is <= hk (a list is sorted, EMPTY-padded)
    for (int l = tid; l < nlist; l += 256) {
        if (at(l, 0) > hk) continue;  // (an L2 hit: loaded in step 1)
        for (int t0 = 0; t0 < k; t0 += 8) {
            uint64_t v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = t0 + u < k ? at(l, t0 + u) : KEY_EMPTY;
            bool more = true;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (v[u] <= hk && v[u] != KEY_EMPTY) {
                    const int pos = atomicAdd(&ccount, 1);
                    if (pos < CAP) cand[pos] = v[u];
                } else {
                    more = false;
                }
            }
            if (!more) break;
        }
    }
    __syncthreads();
    const int nc = ccount;
    if (nc > CAP) {  // block-uniform: the full merge
        merge_partial_lists<CAP>(partial, nlist, nq_total, qi, k, lds, tk);
    } else if (wave == 0) {
        tk.init(as_lds(&lds[0][0]), k);
        for (int j = 0; j < nc; j += 64) {
            tk.reserve(64);
            tk.push(j + lane < nc, j + lane < nc ? cand[j + lane] : KEY_EMPTY);
        }
        tk.compact();
    }
    if (wave == 0) {
        for (int j = lane; j < k; j += 64) {
            const uint64_t key = tk.buf[j];
            RC_EMIT_KEY(key, row_base, row_stride, out_scores[(int64_t)qi * k + j], out_rows[(int64_t)qi * k + j]);
        }
    }
}

// Cross-shard merge: nlists lists of (score, global row) per query.  The key's
// low word is the global row itself (< 2^32), so equal scores order by row
// whatever the row → shard routing (contiguous ranges or round-robin).  Rows
// < 0 are empty slots.
template <int CAP>
__global__ __launch_bounds__(256) void merge_lists_kernel(const float *__restrict__ scores,
                                                         const int64_t *__restrict__ rows, int nlists, int nq,
                                                         int k_in, int k, float *__restrict__ out_scores,
                                                         int64_t *__restrict__ out_rows) {
    __shared__ uint64_t lds[4][CAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = blockIdx.x;
    WaveTopK<CAP> tk;
    tk.init(as_lds(&lds[wave][0]), k);
    const int64_t total = (int64_t)nlists * k_in;
    for (int64_t j0 = (int64_t)wave * 64; j0 < total; j0 += 256) {
        const int64_t j = j0 + lane;
        uint64_t key = KEY_EMPTY;
        bool ok = false;
        if (j < total) {
            const int64_t l = j / k_in, t = j - l * k_in;
            const int64_t src = (l * nq + qi) * k_in + t;
            const int64_t row = rows[src];
            ok = row >= 0;
            key = make_key(scores[src], (uint32_t)row);
        }
        tk.reserve(64);
        tk.push(ok, key);
    }
    tk.compact();
    __syncthreads();
    if (wave == 0) {
        fold_wave_lists<CAP>(&lds[0][0], CAP, tk, k);
        for (int j = lane; j < k; j += 64) {
            const uint64_t key = tk.buf[j];
            RC_EMIT_KEY(key, 0, 1, out_scores[(int64_t)qi * k + j], out_rows[(int64_t)qi * k + j]);
        }
    }
}

// Search over zero rows (an empty shard): every slot is (-inf, -1).
__global__ __launch_bounds__(256) void empty_result_kernel(int64_t n, float *__restrict__ scores, int64_t *__restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    scores[i] = -INFINITY;
    rows[i] = -1;
}

// Paged value gather (rc_sharded_query_host_pages): the local row of each position through a
// slot's page table; an empty slot (position < 0) stays negative, which fetch_kernel answers
// with NaN values.  n_pos bounds the table entries read.
__global__ __launch_bounds__(256) void pages_rows_kernel(const int64_t *__restrict__ pos, int64_t n, const int32_t *__restrict__ pages,
                                                        int64_t n_pos, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pos[i];
    out[i] = (p < 0 || p >= n_pos) ? -1 : (int64_t)pages[p / RC_PAGE_ROWS] * RC_PAGE_ROWS + p % RC_PAGE_ROWS;
}

}  // namespace rc

// ================================================================= host ====
using namespace rc;

struct rc_index {
    std::mutex mu;
    int device = 0;
    int dim = 0;
    int dtype = RC_F32;
    int nch = 1;  // ld = 128 * nch
    int64_t ld = 0;
    int64_t capacity = 0;
    int64_t row_base = 0;    // a search returns row_base + local row * row_stride (shard → global rows)
    int64_t row_stride = 1;
    int ncu = 256;           // compute units of the device (scan grid rounds)
    void *rows = nullptr;
    float *norms = nullptr;
    // int8 filter copy (RC_FILTER_I8): [cap_pad][ld] x8, sx / ex [cap_pad] at i8_slot(row)
    int filter = RC_FILTER_NATIVE;
    int metric = RC_METRIC_COSINE;  // scoring rule of the searches (rc_index_set_metric); storage does not depend on it
    int8_t *rows8 = nullptr;
    float *rsx = nullptr, *rex = nullptr;
    // search workspace
    int ws_nq = 0, ws_k = 0, ws_nblk = 0;
    float *qn = nullptr;
    uint64_t *partial = nullptr;
    unsigned *q1_done = nullptr;    // host-coherent completion word of the polled query1 path
    unsigned q1_seq = 0;
    BatchWs bws;         // batched MFMA search workspace (search_mfma.hip)
    KernelTimer timer;   // scan_topk_kernel launches (bytes)
    KernelTimer gtimer;  // the batched search's filter launches, whichever filter kernel (flops)
    // page tables (rc_index_pages_set), by slot: one device allocation each, doubled when it grows
    struct PageTable {
        int32_t *dev = nullptr;
        int n_pages = 0, cap = 0;
    };
    std::vector<PageTable> tables;
    int64_t *pg_rows = nullptr;  // [pg_rows_cap] local rows of a paged value gather
    int64_t pg_rows_cap = 0;
    // deep top-k (rc_index_search_deep): the score arrays of the queries in flight and the selection's workspace
    float *dscores = nullptr;  // [dscores_cap]
    int64_t dscores_cap = 0;
    DeepSel dsel;
    // sparse-dense hybrid (rc_index_sparse_enable): the store, [width][capacity] slot-major, and the staging of
    // sparse queries and store writes
    SparseStore sparse;
    SparseWs sws;
};

namespace {

constexpr int kNchSet[] = {1, 2, 3, 4, 6, 8, 12, 16};
constexpr int kMaxBlocks = 2048;
constexpr int64_t kSparseWriteSlots = int64_t(1) << 20;  // slots one round of rc_index_sparse_write stages (8 MB)
constexpr int kBatchMinQueries = 8;      // below this the HBM-bound scan wins (1-4 queries per pass)
constexpr int64_t kBatchMinRows = 65536;  // tiny shards: the staged path's fixed cost dominates
// The float8 filter (RC_FILTER_F8) has a corner of its own: the scan it competes with reads half the
// bytes of an f16 scan, and at the two thresholds above that scan wins (16 queries x top-10, wall
// ms per call, filter / scan, tools/f8_filter_micro.py --crossover, profiles/f8_filter/): 70 000 x 256
// 0.331 / 0.232, 70 000 x 512 0.365 / 0.352, 300 000 x 256 0.465 / 0.339, and with 8 queries
// everywhere up to 300 000 x 512.  What decides is how many passes the scan needs, P = ceil(nq /
// queries per pass) (scan_max_qb: 4, 2 or 1 by row width), at about 20 us plus the row bytes each.
// Measured: P = 16 wins from 140 000 rows at every width (1.17-2.2x; at 66 000 x 768, top-100, it
// is 0.91x), P = 8 is at parity from 72 MB of rows and ahead from 230 MB (1.12x; 512 MB: 2.0x).
constexpr int kF8BatchMinPasses = 16;
constexpr int64_t kF8BatchMinRows = 131072;
constexpr int kF8BatchMinPassesLarge = 8;                     // ... with at least
constexpr int64_t kF8BatchMinBytesLarge = int64_t(1) << 28;  // this many bytes of rows
// The metric filter (RC_FILTER_METRIC under dotproduct / euclidean) competes with a scan of one
// query per pass, but at kBatchMinQueries the batched path is behind it up to 131 072 rows (f16,
// top-10, wall ms per call, scan / batched, tools/metric_filter_micro.py, profiles/metric_filter/;
// dotproduct; the euclidean batched search is up to 12 % slower, its scan the same):
//   rows x width      8 queries        16 queries
//    65 536 x 256   0.196 / 0.263    0.377 / 0.337
//    65 536 x 512   0.233 / 0.295    0.454 / 0.369
//    65 536 x 768   0.322 / 0.332    0.632 / 0.410
//   131 072 x 256   0.199 / 0.287    0.385 / 0.369
//   131 072 x 512   0.247 / 0.321    0.481 / 0.397
//   131 072 x 768   0.355 / 0.373    0.701 / 0.460
//   262 144 x 256   0.247 / 0.331    0.479 / 0.422
//   262 144 x 512   0.447 / 0.370    0.872 / 0.448
//   262 144 x 768   0.644 / 0.467    1.273 / 0.561
// 16 queries are ahead everywhere from kBatchMinRows (1.00-2.3x, both metrics); 8 queries from 2^28
// bytes of rows (1.18-1.39x; 9 to 15 queries were not measured and take the 8-query rule).
constexpr int kMetricBatchMinQueries = 16;
constexpr int kMetricBatchMinQueriesLarge = 8;                    // ... with at least
constexpr int64_t kMetricBatchMinBytesLarge = int64_t(1) << 28;  // this many bytes of rows
// The batched search over pages (rc_index_search_pages_ex) competes with the paged scan of the same
// slot (f16 x 512 on a shuffled page list in a 4M-row pool, wall ms per call, median of 5 interleaved
// rounds, paged MFMA / paged scan, tools/paged_batched_micro.py, profiles/paged_batched/; DESIGN.md,
// "Namespaces", row (d) has [min, max] and the dense floor):
//   positions     16 x top-10     16 x top-100    64 x top-10     64 x top-100    1024 x top-10    1024 x top-100
//      65 536   0.380 / 0.361   0.582 / 0.529   0.524 / 1.402   0.823 / 2.047   0.681 / 23.58    1.040 / 33.78
//     262 144   0.496 / 0.550   0.687 / 0.754   0.724 / 2.140   0.986 / 3.032   1.081 / 35.64    1.394 / 48.34
//   1 048 576   0.669 / 1.830   1.020 / 2.208   0.887 / 7.331   1.434 / 8.718   1.755 / 117.1    2.587 / 139.1
// 16 queries over 65 536 positions are behind the scan (its 8 two-query passes are cheaper than the
// staged path's fixed cost); every other measured cell is ahead with its [min, max] wholly below the
// scan's.  RC_SEARCH_AUTO without a mask takes the batched path from the smallest measured corners
// that are: 64 queries from 65 536 positions, 16 queries from 262 144.  17 to 63 queries below
// 262 144 positions were not measured and scan.
constexpr int kPagedBatchMinQueries = 64;
constexpr int64_t kPagedBatchMinPositions = 65536;
constexpr int kPagedBatchMinQueriesLarge = 16;               // ... or with at least
constexpr int64_t kPagedBatchMinPositionsLarge = 262144;    // this many positions on this shard

// Every global row a shard can report must fit the 32-bit row word of the top-k
// keys (merge_lists_kernel) below the all-ones value: row_base + (cap - 1) * stride < 2^32 - 1.
bool row_map_fits(int64_t row_base, int64_t row_stride, int64_t cap) {
    return (double)row_base + (double)(cap - 1) * (double)row_stride < 4294967295.0;
}

// f8 rows are whole 256-element steps (16 lanes x 16 B): an even nch (RowShape::WHOLE)
int pick_nch(int dim, int dtype) {
    const int need = (dim + 127) / 128;
    for (int n : kNchSet)
        if (n >= need && (dtype != RC_F8 || n % 2 == 0)) return n;
    return -1;
}

void ensure_workspace(rc_index *h, int nq, int k) {
    if (nq <= h->ws_nq && k <= h->ws_k) return;
    const int nq2 = std::max(nq, h->ws_nq), k2 = std::max(k, h->ws_k);
    dfree(h->qn);
    dfree(h->partial);
    h->qn = nullptr;
    h->partial = nullptr;
    h->qn = (float *)dmalloc((size_t)nq2 * h->ld * sizeof(float));
    h->partial = (uint64_t *)dmalloc((size_t)kMaxBlocks * nq2 * k2 * sizeof(uint64_t));
    h->ws_nq = nq2;
    h->ws_k = k2;
}

int64_t cap_pad(int64_t capacity) { return (capacity + INDEX_ROW_PAD - 1) / INDEX_ROW_PAD * INDEX_ROW_PAD; }

// refresh the int8 filter copy of rows slots[0..n) (or row0 .. row0 + n) after a write
template <typename T>
void launch_quantize(rc_index *h, const int64_t *slots, int64_t row0, int64_t n, hipStream_t s) {
    if (h->rows8 == nullptr || n == 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>((n + 3) / 4, 256 * 32);
    hipLaunchKernelGGL(quantize_rows_kernel<T>, dim3(grid), dim3(256), 0, s, (const T *)h->rows, h->ld, slots, row0, n,
                       h->capacity, h->rows8, h->rsx, h->rex);
    RC_LAUNCH_CHECK();
}

void free_filter(rc_index *h) {
    dfree(h->rows8);
    dfree(h->rsx);
    dfree(h->rex);
    h->rows8 = nullptr;
    h->rsx = h->rex = nullptr;
    h->filter = RC_FILTER_NATIVE;
}

template <typename T>
void launch_upsert(rc_index *h, const float *vecs, const int64_t *src_idx, int64_t n, const int64_t *slots, hipStream_t s) {
    const unsigned grid = (unsigned)((n + 3) / 4);
    hipLaunchKernelGGL(upsert_kernel<T>, dim3(grid), dim3(256), 0, s, (T *)h->rows, h->norms, h->ld, h->dim, vecs, src_idx,
                       slots, n, h->capacity);
    RC_LAUNCH_CHECK();
    launch_quantize<T>(h, slots, 0, n, s);
}

// rows dst_idx[v] of `to` = rows src_idx[v] of `from`; a null index stands for the staging
// block `stage` on that side (and its list is then null: contiguous).  Refreshes the int8
// filter copy of the written slots, as launch_upsert does: i8_slot's layout keeps one writer.
template <typename T>
void launch_move_rows(rc_index *from, const int64_t *src_idx, rc_index *to, const int64_t *dst_idx, const RowBlock &stage,
                      int64_t n, hipStream_t s) {
    const unsigned grid = (unsigned)std::min<int64_t>((n + 3) / 4, kMaxBlocks);
    hipLaunchKernelGGL(move_rows_kernel<T>, dim3(grid), dim3(256), 0, s, (const T *)(from ? from->rows : stage.rows),
                       (const float *)(from ? from->norms : stage.norms), src_idx, from ? from->capacity : stage.cap,
                       (T *)(to ? to->rows : stage.rows), to ? to->norms : stage.norms, dst_idx,
                       to ? to->capacity : stage.cap, (from ? from : to)->ld, n);
    RC_LAUNCH_CHECK();
    if (to != nullptr) launch_quantize<T>(to, dst_idx, 0, n, s);
}

template <typename T>
void launch_fetch(rc_index *h, const int64_t *slots, int64_t n, float *out, bool stored, hipStream_t s) {
    const unsigned grid = (unsigned)((n + 3) / 4);
    hipLaunchKernelGGL(fetch_kernel<T>, dim3(grid), dim3(256), 0, s, (const T *)h->rows, stored ? nullptr : h->norms, h->ld,
                       h->dim, slots, n, out, h->capacity);
    RC_LAUNCH_CHECK();
}

template <typename T>
void launch_fill(rc_index *h, uint64_t seed, int64_t row0, int64_t n, hipStream_t s) {
    const unsigned grid = (unsigned)std::min<int64_t>((n + 3) / 4, 256 * 32);
    if (grid == 0) return;
    hipLaunchKernelGGL(fill_random_kernel<T>, dim3(grid), dim3(256), 0, s, (T *)h->rows, h->norms, h->ld, h->dim, seed, row0, n);
    RC_LAUNCH_CHECK();
    launch_quantize<T>(h, nullptr, row0, n, s);
}

void launch_scan(rc_index *h, const ScanArgs &a) {
    dispatch_dtype(h->dtype, [&](auto t) { rc::launch_scan<decltype(t)>(a); });
}

void launch_scan_paged(rc_index *h, const ScanArgs &a, const int32_t *pages) {
    const PagedScanArgs p{a, pages};
    dispatch_dtype(h->dtype, [&](auto t) {
        if (a.metric != RC_METRIC_COSINE) rc::launch_scan_paged_metric<decltype(t)>(p);
        else rc::launch_scan_paged<decltype(t)>(p);
    });
}

// Top-k over nlist sorted partial lists per query, one block per query: past MERGE_HEADS_MIN lists
// through the lists' heads (merge_heads_kernel), else over every key (merge_partials_kernel).  The
// same keys either way.
void launch_merge_partials(rc_index *h, const uint64_t *partial, const int *flags, int nlist, int nq, int nq_stride, int k,
                           float *scores, int64_t *rows, hipStream_t s) {
    with_topk_cap(topk_cap(k), [&](auto cap) {
        constexpr int CAP = decltype(cap)::value;
        if (nlist >= MERGE_HEADS_MIN)
            hipLaunchKernelGGL(merge_heads_kernel<CAP>, dim3(nq), dim3(256), 0, s, partial, nlist, nq_stride, k, h->row_base,
                               h->row_stride, flags, scores, rows);
        else
            hipLaunchKernelGGL(merge_partials_kernel<CAP>, dim3(nq), dim3(256), 0, s, partial, nlist, nq_stride, k, h->row_base,
                               h->row_stride, flags, scores, rows);
    });
    RC_LAUNCH_CHECK();
}

// mask (optional): the row-eligibility bitmap of rc_index_search_masked; the masked scan kernels.
// pages (optional): a slot's page table (rc_index_search_pages); n_rows, the blocks' ranges, the
// mask and the returned rows are then positions, and the paged scan kernels run over the same
// block shape, so the partial lists are those of a dense index of the positions.
void scan_search(rc_index *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask, float *scores,
                 int64_t *out_rows, hipStream_t s, const int32_t *pages = nullptr) {
    // queries per scan pass: a power of two the kernel is instantiated for (1, 2, 4)
    int qb = 1;
    while (qb * 2 <= std::min(nq, scan_max_qb(h->nch, k, mask != nullptr, h->metric))) qb *= 2;
    const int nq_pad = (nq + qb - 1) / qb * qb;  // every scan pass runs qb real-or-zero query slots
    ensure_workspace(h, nq_pad, k);  // (the scan normalises the queries itself: no separate launch)
    int nblk = (int)std::min<int64_t>(kMaxBlocks, std::max<int64_t>(1, (n_rows + 511) / 512));
    // past one round of resident blocks (4 per CU), whole rounds: 1M rows were 1954 blocks = 1.9
    // rounds, a tail of CUs with one block fewer; 1024 blocks of ~1000 rows are one round (and a
    // merge over half the lists)
    const int round_blocks = 4 * h->ncu;
    if (nblk > round_blocks) nblk = nblk / round_blocks * round_blocks;
    int64_t rpb = (n_rows + nblk - 1) / nblk;
    rpb = ((rpb + 31) / 32) * 32;
    if (rpb == 0) rpb = 32;
    nblk = (int)std::max<int64_t>(1, (n_rows + rpb - 1) / rpb);
    const double bytes = (double)n_rows * h->ld * dtype_size(h->dtype);
    if (h->timer.enabled) h->timer.create();
    for (int q0 = 0; q0 < nq_pad; q0 += qb) {
        const int slot = h->timer.begin(s);
        ScanArgs a{h->rows, h->ld, h->nch, n_rows, rpb, nblk, h->qn, q0, qb, nq_pad, k, h->partial, s};
        a.qraw = queries;
        a.dim = h->dim;
        a.nq_real = nq;
        a.mask = mask;
        a.metric = h->metric;  // non-cosine: the metric kernels, which also read the norms
        a.norms = h->norms;
        if (pages != nullptr) launch_scan_paged(h, a, pages);
        else launch_scan(h, a);
        h->timer.end(slot, s, bytes);
    }
    launch_merge_partials(h, h->partial, nullptr, nblk, nq, nq_pad, k, scores, out_rows, s);
}

// bytes per element of BatchWs::qh: the storage dtype's, and two byte planes (q_hi, q_lo) on a float8 index
int batch_query_bytes(const rc_index *h) { return h->dtype == RC_F8 ? 2 : (int)dtype_size(h->dtype); }

// Batched MFMA search, then — still on the device, no host synchronisation —
// the exact scan for every query whose candidates overflowed: scan_topk_kernel
// in fallback mode (blocks early-exit for unflagged queries) over the batched
// path's normalised queries (wave_inv_norm / RC_UNIT_ELEM, the scan's own normalisation),
// and merge_partials_kernel over the flagged queries' partial lists.
// With a mask the rescoring drops ineligible candidates (search_mfma.hip) and the
// fallback is the masked scan; the merge is the same.  mask_filter (RC_SEARCH_MFMA_MASKED): the
// filter kernels apply the mask as well, in their MASKED forms.
// pages (optional): a slot's page table (rc_index_search_pages_ex); n_rows, the mask and the returned
// rows are then positions, the filter and rescore kernels their PAGED forms (search_mfma_paged.hip),
// and the fallback the paged scan's fallback form (scan_paged.h), each query normalised from the raw
// queries as every paged scan does.
void batched_search_exact(rc_index *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask,
                          bool mask_filter, float *scores, int64_t *out_rows, hipStream_t s, const int32_t *pages = nullptr) {
    h->bws.ensure(nq, k, h->ld, batch_query_bytes(h));
    BatchPlan p{h->rows, h->dtype, h->dim, h->nch, h->ld, n_rows, h->row_base, h->row_stride, queries, nq, k, scores, out_rows};
    p.f8_filter = h->filter == RC_FILTER_F8;
    p.rows8 = h->rows8;
    p.rsx = h->rsx;
    p.rex = h->rex;
    p.mask = mask;
    p.mask_filter = mask_filter && mask != nullptr;
    p.metric = h->metric;  // non-cosine (RC_FILTER_METRIC): the filter and rescore kernels' metric forms
    p.norms = h->norms;
    p.pages = pages;
    if (h->gtimer.enabled) h->gtimer.create();
    batched_search(p, h->bws, s, h->gtimer.enabled ? &h->gtimer : nullptr);
    int nblk = (int)std::min<int64_t>(h->bws.fb_blocks, std::max<int64_t>(1, (n_rows + 511) / 512));
    int64_t rpb = (n_rows + nblk - 1) / nblk;
    rpb = std::max<int64_t>(32, (rpb + 31) / 32 * 32);
    nblk = (int)std::max<int64_t>(1, (n_rows + rpb - 1) / rpb);
    ScanArgs a{h->rows, h->ld, h->nch, n_rows, rpb, nblk, h->bws.qn, 0, 1, nq, k, h->bws.fb_partial, s};
    a.flags = h->bws.flags;
    a.grid_y = std::min(nq, FB_QSTRIDE);
    a.mask = mask;
    if (h->metric != RC_METRIC_COSINE || pages != nullptr) {  // the metric fallback kernel (scan_metric.h) and the paged
        a.metric = h->metric;                                 // ones (scan_paged.h): raw queries, as every such scan
        a.norms = h->norms;
        a.qraw = queries;
        a.dim = h->dim;
        a.nq_real = nq;
    }
    if (pages != nullptr) launch_scan_paged(h, a, pages);
    else launch_scan(h, a);
    launch_merge_partials(h, h->bws.fb_partial, h->bws.flags, nblk, nq, nq, k, scores, out_rows, s);
}

void empty_search(int nq, int k, float *scores, int64_t *out_rows, hipStream_t s) {
    const int64_t n = (int64_t)nq * k;
    hipLaunchKernelGGL(empty_result_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, scores, out_rows);
    RC_LAUNCH_CHECK();
}

// The deep top-k's score pass (deep_scores.h) over scan_search's block shape: the f32 score of nq
// raw queries against rows (pages: positions) [0, n), out[q * n + r].  n >= 1.
void deep_score_pass(rc_index *h, const float *queries, int nq, int64_t n, const int32_t *pages, float *out, hipStream_t s) {
    int nblk = (int)std::min<int64_t>(kMaxBlocks, std::max<int64_t>(1, (n + 511) / 512));
    const int round_blocks = 4 * h->ncu;
    if (nblk > round_blocks) nblk = nblk / round_blocks * round_blocks;
    int64_t rpb = (n + nblk - 1) / nblk;
    rpb = std::max<int64_t>(32, (rpb + 31) / 32 * 32);
    nblk = (int)std::max<int64_t>(1, (n + rpb - 1) / rpb);
    const DeepScoreArgs a{h->rows, h->norms, h->ld, h->nch, h->dim, n, rpb, nblk, queries, nq, h->metric, pages, out, s};
    dispatch_dtype(h->dtype, [&](auto t) { launch_deep_scores<decltype(t)>(a); });
}

// rc_index_search_deep's body (caller holds h->mu, the device is current): the k best of rows
// (pages: positions) [0, n) per query, in chunks of deep_chunk_queries() queries: the chunk's
// score pass, then every selection round over its scores.  out_keys (sharded.hip: [nq][k] keys
// carrying global rows) or, when it is null, scores / out_rows through the emit kernel.
// after (the hybrid searches; null for the deep ones): a step between a chunk's score pass and its selection.
void deep_search_locked(rc_index *h, const float *queries, int nq, int64_t n, int k, const uint32_t *mask, const int32_t *pages,
                        uint64_t *out_keys, float *scores, int64_t *out_rows, hipStream_t s, const DeepAfterScores *after = nullptr) {
    if (n == 0) {  // an empty shard: every slot is empty
        if (out_keys != nullptr) RC_HIP(hipMemsetAsync(out_keys, 0xff, (size_t)nq * k * sizeof(uint64_t), s));
        else empty_search(nq, k, scores, out_rows, s);
        return;
    }
    const int qc = deep_chunk_queries(nq, n);
    if ((int64_t)qc * n > h->dscores_cap) {
        dfree(h->dscores);
        h->dscores = nullptr;
        h->dscores_cap = 0;
        h->dscores = (float *)dmalloc((size_t)qc * n * sizeof(float));
        h->dscores_cap = (int64_t)qc * n;
    }
    h->dsel.ensure(qc, out_keys != nullptr ? 0 : (int64_t)qc * k);
    for (int q0 = 0; q0 < nq; q0 += qc) {
        const int m = std::min(qc, nq - q0);
        deep_score_pass(h, queries + (int64_t)q0 * h->dim, m, n, pages, h->dscores, s);
        if (after != nullptr) (*after)(q0, m, h->dscores, s);
        DeepStream st;
        st.scores = h->dscores;
        st.n = n;
        st.row_base = h->row_base;
        st.row_stride = h->row_stride;
        st.mask = mask;
        uint64_t *ko = out_keys != nullptr ? out_keys + (int64_t)q0 * k : h->dsel.keys;
        deep_select_rounds(st, h->dsel, m, k, ko, s);
        if (out_keys == nullptr) deep_emit(ko, (int64_t)m * k, scores + (int64_t)q0 * k, out_rows + (int64_t)q0 * k, s);
    }
}

// The hybrid searches' step after the score pass (caller holds h->mu, the device is current): checks
// done, the sparse queries of the whole call are staged on `s` and the step adds a chunk's terms
// over rows (pages: positions) [0, n).  No query holds an entry: no step (null), the deep search as it is.
DeepAfterScores sparse_step(rc_index *h, const SparseQueries &sq, int nq, int64_t n, const int32_t *pages, hipStream_t s) {
    if (sq.off[nq] == 0 || n == 0) return nullptr;
    h->sws.stage_queries(sq, nq, s);
    return [h, n, pages](int q0, int m, float *scores, hipStream_t st) {
        const SparseAddArgs a{h->sparse.idx, h->sparse.val, h->sparse.width, h->capacity, h->sws.off_d, h->sws.idx_d, h->sws.val_d,
                              q0,            m,             n,               pages,       scores,       st};
        launch_sparse_add(a);
    };
}

// What every hybrid call checks of its sparse queries before any device call (caller holds h->mu).
void check_hybrid(const rc_index *h, const SparseQueries &sq, int nq) {
    RC_REQUIRE(h->sparse.width > 0, RC_ERR_INVALID, "this index has no sparse store (rc_index_sparse_enable)");
    RC_REQUIRE(h->metric == RC_METRIC_DOT, RC_ERR_INVALID, "sparse-dense hybrid scores need the dotproduct metric");
    sparse_check_queries(sq, nq);
}

}  // namespace

namespace rc {
// Internal (sharded.hip): upsert vectors vecs[src_idx[i]] into local rows rows[i].
void index_upsert_gather(rc_index *h, const float *vecs, const int64_t *src_idx, int64_t n, const int64_t *rows,
                         hipStream_t s) {
    if (n == 0) return;
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceScope ds(h->device);
    dispatch_dtype(h->dtype, [&](auto t) { launch_upsert<decltype(t)>(h, vecs, src_idx, n, rows, s); });
}

// Internal (sharded.hip) and rc_index_move_rows: move n stored rows from `from` (rows src_idx[i])
// to `to` (rows dst_idx[i]) on the current stream `s` of their device.  One of the two may be
// null: that side is the staging block `stage` (same device), read or written contiguously from
// its row 0, and its list is null (pack / unpack).  from == to moves inside a shard; two
// different handles must share a device and a layout (two shards of one GPU).
void index_move_rows(rc_index *from, const int64_t *src_idx, rc_index *to, const int64_t *dst_idx, const RowBlock &stage,
                     int64_t n, hipStream_t s) {
    if (n == 0) return;
    rc_index *any = from ? from : to;
    RC_REQUIRE(any != nullptr, RC_ERR_INVALID, "null index");
    RC_REQUIRE((from != nullptr) == (src_idx != nullptr) && (to != nullptr) == (dst_idx != nullptr), RC_ERR_INVALID,
               "a row list goes with an index, none with the staging block");
    if (from && to && from != to)
        RC_REQUIRE(from->device == to->device && from->ld == to->ld && from->dtype == to->dtype, RC_ERR_INVALID,
                   "a direct move needs two shards of one device and one layout");
    std::unique_lock<std::mutex> l1, l2;
    if (from && to && from != to) {
        std::lock(from->mu, to->mu);
        l1 = std::unique_lock<std::mutex>(from->mu, std::adopt_lock);
        l2 = std::unique_lock<std::mutex>(to->mu, std::adopt_lock);
    } else {
        l1 = std::unique_lock<std::mutex>(any->mu);
    }
    DeviceScope ds(any->device);
    dispatch_dtype(any->dtype, [&](auto t) { launch_move_rows<decltype(t)>(from, src_idx, to, dst_idx, stage, n, s); });
}

// Internal (sharded.hip, rc_sharded_query_host): one query as ONE launch (query1_kernel) —
// normalise, scan, merge, gather values — writing scores [k], rows [k] and (with_values)
// values [k][dim] to out_* (host-mapped memory is fine: nothing is copied back).  Returns
// false, enqueuing nothing, when the shape is outside the kernel's range (the caller takes
// the multi-kernel path).  n_rows >= 1.
bool index_query1(rc_index *h, const float *query, int64_t n_rows, int k, int with_values, float *out_scores,
                  int64_t *out_rows, float *out_values, hipStream_t s, volatile unsigned **done, unsigned *seq) {
    if (h->dim > QUERY1_MAX_DIM || h->nch > 6 || topk_cap(k) > 256 || n_rows < 1 || n_rows > QUERY1_MAX_ROWS) return false;
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceScope ds(h->device);
    ensure_workspace(h, 1, k);
    Query1Args a{};
    a.rows = h->rows;
    a.norms = h->norms;
    a.ld = h->ld;
    a.dim = h->dim;
    a.nch = h->nch;
    a.n_rows = n_rows;
    // >= 64 rows a block (two passes of the block's 32-row step), at most QUERY1_MAX_BLOCKS lists
    int64_t rpb = std::max<int64_t>(64, (n_rows + QUERY1_MAX_BLOCKS - 1) / QUERY1_MAX_BLOCKS);
    rpb = (rpb + 31) / 32 * 32;
    a.rows_per_block = rpb;
    a.nblk = (int)((n_rows + rpb - 1) / rpb);
    a.k = k;
    a.with_values = with_values;
    a.metric = h->metric;
    a.row_base = h->row_base;
    a.row_stride = h->row_stride;
    a.partial = h->partial;
    a.out_scores = out_scores;
    a.out_rows = out_rows;
    a.out_values = out_values;
    if (done != nullptr) {  // the caller polls a host-coherent completion word (see spin_until)
        if (h->q1_done == nullptr) {
            RC_HIP(hipHostMalloc((void **)&h->q1_done, 64, hipHostMallocCoherent));
            *h->q1_done = 0u;
        }
        a.done = h->q1_done;
        a.seq = ++h->q1_seq;
        if (a.seq == 0u) a.seq = ++h->q1_seq;  // 0 is the initial word
        *done = h->q1_done;
        *seq = a.seq;
    }
    std::memcpy(a.q, query, (size_t)h->dim * sizeof(float));
    dispatch_dtype(h->dtype, [&](auto t) { launch_query1<decltype(t)>(a, s); });
    return true;
}

// The table of a slot, or an error (caller holds h->mu).
static const rc_index::PageTable &page_table(const rc_index *h, int slot) {
    RC_REQUIRE(slot >= 0 && slot < (int)h->tables.size() && h->tables[slot].n_pages > 0, RC_ERR_INVALID,
               "unknown slot (no page table was set for it)");
    return h->tables[slot];
}

// Internal (sharded.hip, rc_sharded_query_host_pages): the values of the positions pos[0..n)
// (device; < 0 = empty: NaN) of a slot, as rc_index_fetch gives them, on stream `s`.
void index_fetch_pages(rc_index *h, int slot, int64_t n_pos, const int64_t *pos, int64_t n, float *out, hipStream_t s) {
    if (n == 0) return;
    std::lock_guard<std::mutex> lk(h->mu);
    const rc_index::PageTable &t = page_table(h, slot);
    RC_REQUIRE(n_pos >= 0 && n_pos <= (int64_t)t.n_pages * RC_PAGE_ROWS, RC_ERR_INVALID, "n_pos beyond the slot's pages");
    DeviceScope ds(h->device);
    if (n > h->pg_rows_cap) {
        RC_HIP(hipDeviceSynchronize());  // no gather may still read the old list
        dfree(h->pg_rows);
        h->pg_rows = nullptr;
        h->pg_rows_cap = 0;
        h->pg_rows = (int64_t *)dmalloc((size_t)n * sizeof(int64_t));
        h->pg_rows_cap = n;
    }
    hipLaunchKernelGGL(pages_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pos, n, t.dev, n_pos, h->pg_rows);
    RC_LAUNCH_CHECK();
    dispatch_dtype(h->dtype, [&](auto tt) { launch_fetch<decltype(tt)>(h, h->pg_rows, n, out, false, s); });
}

// Internal (sharded.hip, rc_sharded_search_deep): a shard's own deep top-k as keys [nq][k] that
// carry global rows (slot >= 0: global positions of that slot over [0, n) local positions),
// KEY_EMPTY past the eligible rows, on stream `s`.  mask: device bitmap over the local rows /
// positions, or null.  The caller has checked nq, k and the buffers.
// sq (rc_sharded_search_hybrid): the call's sparse queries, already checked; null: the deep search.
void index_search_deep_keys(rc_index *h, const float *queries, int nq, int64_t n, int k, const uint32_t *mask, int slot,
                            uint64_t *out_keys, hipStream_t s, const SparseQueries *sq) {
    std::lock_guard<std::mutex> lk(h->mu);
    const int32_t *pages = nullptr;
    if (slot >= 0) {
        const rc_index::PageTable &t = page_table(h, slot);
        RC_REQUIRE(n >= 0 && n <= (int64_t)t.n_pages * RC_PAGE_ROWS, RC_ERR_INVALID, "n_pos beyond the slot's pages");
        pages = t.dev;
    } else {
        RC_REQUIRE(n >= 0 && n <= h->capacity, RC_ERR_INVALID, "n_rows out of range");
    }
    if (sq != nullptr) RC_REQUIRE(h->sparse.width > 0, RC_ERR_INVALID, "this index has no sparse store (rc_index_sparse_enable)");
    DeviceScope ds(h->device);
    const DeepAfterScores step = sq != nullptr ? sparse_step(h, *sq, nq, n, pages, s) : nullptr;
    deep_search_locked(h, queries, nq, n, k, mask, pages, out_keys, nullptr, nullptr, s, step ? &step : nullptr);
}
}  // namespace rc

extern "C" {

const char *rc_last_error(void) { return g_last_error.c_str(); }
int rc_abi_version(void) { return RC_ABI_VERSION; }
int64_t rc_alloc_count(void) { return g_alloc_count.load(std::memory_order_relaxed); }

int rc_index_create(int device, int dim, int dtype, int64_t capacity, int64_t row_base, rc_index **out) {
    return guard([&] {
        RC_REQUIRE(out != nullptr, RC_ERR_INVALID, "out is NULL");
        RC_REQUIRE(dim > 0, RC_ERR_INVALID, "dimension must be positive");
        RC_REQUIRE(dtype == RC_F32 || dtype == RC_F16 || dtype == RC_BF16 || dtype == RC_F8, RC_ERR_INVALID,
                   "dtype must be RC_F32/RC_F16/RC_BF16/RC_F8");
        RC_REQUIRE(capacity > 0 && capacity < (int64_t(1) << 32), RC_ERR_INVALID, "capacity must be in [1, 2^32)");
        RC_REQUIRE(row_base >= 0 && row_map_fits(row_base, 1, capacity), RC_ERR_INVALID,
                   "row_base + capacity must stay below 2^32 - 1 (global rows key the top-k merge)");
        const int nch = pick_nch(dim, dtype);
        RC_REQUIRE(nch > 0, RC_ERR_UNSUPPORTED, "dimension > 2048 is not supported");
        DeviceScope ds(device);
        auto *h = new rc_index();
        h->device = device;
        h->dim = dim;
        h->dtype = dtype;
        h->nch = nch;
        h->ld = 128LL * nch;
        h->capacity = capacity;
        h->row_base = row_base;
        try {
            RC_HIP(hipDeviceGetAttribute(&h->ncu, hipDeviceAttributeMultiprocessorCount, device));
            // whole 256-row tiles: the batched search reads row tiles without a bounds check
            const int64_t cap_pad = (capacity + INDEX_ROW_PAD - 1) / INDEX_ROW_PAD * INDEX_ROW_PAD;
            h->rows = dmalloc((size_t)cap_pad * h->ld * dtype_size(dtype));
            h->norms = (float *)dmalloc((size_t)capacity * sizeof(float));
            RC_HIP(hipMemset(h->rows, 0, (size_t)cap_pad * h->ld * dtype_size(dtype)));
            RC_HIP(hipMemset(h->norms, 0, (size_t)capacity * sizeof(float)));
            ensure_workspace(h, 4, 16);
        } catch (...) {
            dfree(h->rows);
            dfree(h->norms);
            dfree(h->qn);
            dfree(h->partial);
            delete h;
            throw;
        }
        *out = h;
    });
}

int rc_index_destroy(rc_index *h) {
    return guard([&] {
        if (!h) return;
        DeviceScope ds(h->device);
        h->timer.destroy();
        h->gtimer.destroy();
        h->bws.release();
        free_filter(h);
        dfree(h->rows);
        dfree(h->norms);
        dfree(h->qn);
        dfree(h->partial);
        if (h->q1_done != nullptr) (void)hipHostFree(h->q1_done);
        for (auto &t : h->tables) dfree(t.dev);
        dfree(h->pg_rows);
        dfree(h->dscores);
        h->dsel.release();
        dfree(h->sparse.idx);
        dfree(h->sparse.val);
        h->sws.release();
        delete h;
    });
}

int rc_index_info(const rc_index *h, int *dim, int *dtype, int64_t *capacity, int64_t *ld) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        if (dim) *dim = h->dim;
        if (dtype) *dtype = h->dtype;
        if (capacity) *capacity = h->capacity;
        if (ld) *ld = h->ld;
    });
}

int rc_index_data(const rc_index *h, void **rows_dev, float **norms_dev) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        if (rows_dev) *rows_dev = h->rows;
        if (norms_dev) *norms_dev = h->norms;
    });
}

int rc_index_set_row_map(rc_index *h, int64_t row_base, int64_t row_stride) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(row_base >= 0 && row_stride >= 1, RC_ERR_INVALID, "row_base must be >= 0 and row_stride >= 1");
        std::lock_guard<std::mutex> lk(h->mu);
        RC_REQUIRE(row_map_fits(row_base, row_stride, h->capacity), RC_ERR_INVALID,
                   "row map exceeds 2^32 - 1 global rows (row_base + (capacity - 1) * row_stride)");
        h->row_base = row_base;
        h->row_stride = row_stride;
    });
}

int rc_index_grow(rc_index *h, int64_t new_capacity, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(new_capacity < (int64_t(1) << 32), RC_ERR_INVALID, "capacity must be < 2^32");
        std::lock_guard<std::mutex> lk(h->mu);
        if (new_capacity <= h->capacity) return;
        RC_REQUIRE(row_map_fits(h->row_base, h->row_stride, new_capacity), RC_ERR_INVALID,
                   "grown capacity exceeds 2^32 - 1 global rows under this shard's row map");
        DeviceScope ds(h->device);
        hipStream_t s = (hipStream_t)stream;
        const size_t rb = (size_t)h->ld * dtype_size(h->dtype);
        const int64_t old_pad = (h->capacity + INDEX_ROW_PAD - 1) / INDEX_ROW_PAD * INDEX_ROW_PAD;
        const int64_t new_pad = (new_capacity + INDEX_ROW_PAD - 1) / INDEX_ROW_PAD * INDEX_ROW_PAD;
        void *rows = dmalloc((size_t)new_pad * rb);
        float *norms = nullptr;
        int8_t *rows8 = nullptr;
        float *rsx = nullptr, *rex = nullptr;
        uint32_t *sp_idx = nullptr;
        float *sp_val = nullptr;
        try {
            norms = (float *)dmalloc((size_t)new_capacity * sizeof(float));
            RC_HIP(hipMemcpyAsync(rows, h->rows, (size_t)old_pad * rb, hipMemcpyDeviceToDevice, s));
            RC_HIP(hipMemsetAsync((uint8_t *)rows + (size_t)old_pad * rb, 0, (size_t)(new_pad - old_pad) * rb, s));
            RC_HIP(hipMemcpyAsync(norms, h->norms, (size_t)h->capacity * sizeof(float), hipMemcpyDeviceToDevice, s));
            RC_HIP(hipMemsetAsync(norms + h->capacity, 0, (size_t)(new_capacity - h->capacity) * sizeof(float), s));
            if (h->rows8) {  // the filter copy keeps its slots (i8_slot is position-stable)
                const size_t rb8 = (size_t)h->ld;
                rows8 = (int8_t *)dmalloc((size_t)new_pad * rb8);
                rsx = (float *)dmalloc((size_t)new_pad * sizeof(float));
                rex = (float *)dmalloc((size_t)new_pad * sizeof(float));
                RC_HIP(hipMemcpyAsync(rows8, h->rows8, (size_t)old_pad * rb8, hipMemcpyDeviceToDevice, s));
                RC_HIP(hipMemsetAsync(rows8 + (size_t)old_pad * rb8, 0, (size_t)(new_pad - old_pad) * rb8, s));
                RC_HIP(hipMemcpyAsync(rsx, h->rsx, (size_t)old_pad * sizeof(float), hipMemcpyDeviceToDevice, s));
                RC_HIP(hipMemsetAsync(rsx + old_pad, 0, (size_t)(new_pad - old_pad) * sizeof(float), s));
                RC_HIP(hipMemcpyAsync(rex, h->rex, (size_t)old_pad * sizeof(float), hipMemcpyDeviceToDevice, s));
                RC_HIP(hipMemsetAsync(rex + old_pad, 0, (size_t)(new_pad - old_pad) * sizeof(float), s));
            }
            if (h->sparse.width > 0) {  // the sparse store keeps its rows; the new ones are padding
                sp_idx = (uint32_t *)dmalloc((size_t)h->sparse.width * new_capacity * sizeof(uint32_t));
                sp_val = (float *)dmalloc((size_t)h->sparse.width * new_capacity * sizeof(float));
                launch_sparse_regrow(h->sparse, h->capacity, sp_idx, sp_val, new_capacity, s);
            }
            RC_HIP(hipStreamSynchronize(s));  // work queued earlier on other streams is the caller's to order
        } catch (...) {
            dfree(sp_idx);
            dfree(sp_val);
            dfree(rows);
            dfree(norms);
            dfree(rows8);
            dfree(rsx);
            dfree(rex);
            throw;
        }
        RC_HIP(hipDeviceSynchronize());  // no kernel may still read the old buffers
        dfree(h->rows);
        dfree(h->norms);
        h->rows = rows;
        h->norms = norms;
        if (h->rows8) {
            dfree(h->rows8);
            dfree(h->rsx);
            dfree(h->rex);
            h->rows8 = rows8;
            h->rsx = rsx;
            h->rex = rex;
        }
        if (h->sparse.width > 0) {
            dfree(h->sparse.idx);
            dfree(h->sparse.val);
            h->sparse.idx = sp_idx;
            h->sparse.val = sp_val;
        }
        h->capacity = new_capacity;
    });
}

int rc_index_reserve(rc_index *h, int max_nq, int max_k) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(max_nq > 0 && max_k > 0 && max_k <= RC_TOPK_MAX, RC_ERR_INVALID, "bad reserve sizes");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        ensure_workspace(h, max_nq, max_k);
    });
}

int rc_index_set_filter(rc_index *h, int kind, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(kind == RC_FILTER_NATIVE || kind == RC_FILTER_I8 || kind == RC_FILTER_F8 || kind == RC_FILTER_METRIC,
                   RC_ERR_INVALID, "filter must be RC_FILTER_NATIVE, RC_FILTER_I8, RC_FILTER_F8 or RC_FILTER_METRIC");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        hipStream_t s = (hipStream_t)stream;
        if (kind == h->filter) return;
        if (kind == RC_FILTER_NATIVE) {
            RC_HIP(hipDeviceSynchronize());  // no search may still read the copy
            free_filter(h);
            return;
        }
        if (kind == RC_FILTER_METRIC) {  // allocates nothing: the native filter kernels and their metric forms
            RC_REQUIRE(h->dtype == RC_F16 || h->dtype == RC_BF16, RC_ERR_UNSUPPORTED,
                       "the metric filter's GEMM reads stored f16 / bf16 rows: it needs an f16 or bf16 index");
            RC_HIP(hipDeviceSynchronize());
            free_filter(h);  // an int8 copy goes, as on a switch to RC_FILTER_NATIVE
            h->filter = RC_FILTER_METRIC;
            return;
        }
        if (kind == RC_FILTER_F8) {  // allocates nothing: the filter GEMM reads the stored rows
            RC_REQUIRE(h->dtype == RC_F8, RC_ERR_UNSUPPORTED, "the float8 filter reads stored float8 rows: it needs a float8 index");
            RC_REQUIRE(h->metric == RC_METRIC_COSINE, RC_ERR_UNSUPPORTED,
                       "the float8 filter serves the batched MFMA search, which is cosine-only");
            RC_REQUIRE(f8_filter_supported(h->ld), RC_ERR_UNSUPPORTED,
                       "the float8 filter needs a row width (dim rounded up to 256) of 256, 512 or 768");
            h->filter = RC_FILTER_F8;  // (h->rows8 is null: the int8 copy is refused on a float8 index)
            return;
        }
        RC_REQUIRE(h->metric == RC_METRIC_COSINE, RC_ERR_UNSUPPORTED,
                   "the int8 filter serves the batched MFMA search, which is cosine-only");
        // its bound assumes ||x̂|| <= 1.01; an f8 row's norm is off by up to 2^-4 relative
        RC_REQUIRE(h->dtype != RC_F8, RC_ERR_UNSUPPORTED,
                   "the int8 filter is not available on a float8 index (its batched search is RC_FILTER_F8)");
        RC_REQUIRE(i8_filter_supported(h->ld), RC_ERR_UNSUPPORTED,
                   "the int8 filter needs a row width (dim rounded up to 128) of 256, 512 or 768");
        const int64_t pad = cap_pad(h->capacity);
        try {
            h->rows8 = (int8_t *)dmalloc((size_t)pad * h->ld);
            h->rsx = (float *)dmalloc((size_t)pad * sizeof(float));
            h->rex = (float *)dmalloc((size_t)pad * sizeof(float));
            RC_HIP(hipMemsetAsync(h->rows8, 0, (size_t)pad * h->ld, s));
            RC_HIP(hipMemsetAsync(h->rsx, 0, (size_t)pad * sizeof(float), s));
            RC_HIP(hipMemsetAsync(h->rex, 0, (size_t)pad * sizeof(float), s));
            dispatch_dtype(h->dtype, [&](auto t) { launch_quantize<decltype(t)>(h, nullptr, 0, h->capacity, s); });
            RC_HIP(hipStreamSynchronize(s));
        } catch (...) {
            free_filter(h);
            throw;
        }
        h->filter = RC_FILTER_I8;
    });
}

int rc_index_get_filter(const rc_index *h, int *kind) {
    return guard([&] {
        RC_REQUIRE(h && kind, RC_ERR_INVALID, "null argument");
        *kind = h->filter;
    });
}

int rc_index_set_metric(rc_index *h, int metric) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(metric == RC_METRIC_COSINE || metric == RC_METRIC_DOT || metric == RC_METRIC_EUCLIDEAN, RC_ERR_INVALID,
                   "metric must be RC_METRIC_COSINE, RC_METRIC_DOT or RC_METRIC_EUCLIDEAN");
        std::lock_guard<std::mutex> lk(h->mu);
        RC_REQUIRE(metric == RC_METRIC_COSINE || h->filter == RC_FILTER_NATIVE || h->filter == RC_FILTER_METRIC, RC_ERR_UNSUPPORTED,
                   "a non-cosine metric on an index with the int8 filter copy or the float8 filter (those filters are cosine-only)");
        h->metric = metric;  // no device call: searches already enqueued took the metric they were launched with
    });
}

int rc_index_get_metric(const rc_index *h, int *metric) {
    return guard([&] {
        RC_REQUIRE(h && metric, RC_ERR_INVALID, "null argument");
        *metric = h->metric;
    });
}

int rc_index_upsert(rc_index *h, const float *vecs, int64_t n, const int64_t *rows, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(n >= 0, RC_ERR_INVALID, "negative count");
        if (n == 0) return;
        RC_REQUIRE(vecs && rows, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        dispatch_dtype(h->dtype, [&](auto t) { launch_upsert<decltype(t)>(h, vecs, nullptr, n, rows, (hipStream_t)stream); });
    });
}

int rc_index_move_rows(rc_index *h, const int64_t *src_rows, const int64_t *dst_rows, int64_t n, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(n >= 0, RC_ERR_INVALID, "negative count");
        if (n == 0) return;
        RC_REQUIRE(src_rows && dst_rows, RC_ERR_INVALID, "null buffer");
        index_move_rows(h, src_rows, h, dst_rows, RowBlock{}, n, (hipStream_t)stream);
    });
}

int rc_index_fetch(rc_index *h, const int64_t *rows, int64_t n, float *out, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(n >= 0, RC_ERR_INVALID, "negative count");
        if (n == 0) return;
        RC_REQUIRE(rows && out, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        dispatch_dtype(h->dtype, [&](auto t) { launch_fetch<decltype(t)>(h, rows, n, out, false, (hipStream_t)stream); });
    });
}

int rc_index_fetch_stored(rc_index *h, const int64_t *rows, int64_t n, float *out, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(n >= 0, RC_ERR_INVALID, "negative count");
        if (n == 0) return;
        RC_REQUIRE(rows && out, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        dispatch_dtype(h->dtype, [&](auto t) { launch_fetch<decltype(t)>(h, rows, n, out, true, (hipStream_t)stream); });
    });
}

int rc_index_fill_random(rc_index *h, uint64_t seed, int64_t row0, int64_t n, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(row0 >= 0 && n >= 0 && row0 + n <= h->capacity, RC_ERR_INVALID, "rows out of capacity");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        dispatch_dtype(h->dtype, [&](auto t) { launch_fill<decltype(t)>(h, seed, row0, n, (hipStream_t)stream); });
    });
}

int rc_index_export(rc_index *h, int64_t row0, int64_t n, void *rows_out, float *norms_out, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(row0 >= 0 && n >= 0 && row0 + n <= h->capacity, RC_ERR_INVALID, "rows out of capacity");
        if (n == 0) return;
        RC_REQUIRE(rows_out && norms_out, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        const size_t rb = (size_t)h->ld * dtype_size(h->dtype);
        hipStream_t s = (hipStream_t)stream;
        RC_HIP(hipMemcpyAsync(rows_out, (const uint8_t *)h->rows + (size_t)row0 * rb, (size_t)n * rb, hipMemcpyDefault, s));
        RC_HIP(hipMemcpyAsync(norms_out, h->norms + row0, (size_t)n * sizeof(float), hipMemcpyDefault, s));
    });
}

int rc_index_import(rc_index *h, int64_t row0, int64_t n, const void *rows_in, const float *norms_in, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(row0 >= 0 && n >= 0 && row0 + n <= h->capacity, RC_ERR_INVALID, "rows out of capacity");
        if (n == 0) return;
        RC_REQUIRE(rows_in && norms_in, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        const size_t rb = (size_t)h->ld * dtype_size(h->dtype);
        hipStream_t s = (hipStream_t)stream;
        RC_HIP(hipMemcpyAsync((uint8_t *)h->rows + (size_t)row0 * rb, rows_in, (size_t)n * rb, hipMemcpyDefault, s));
        RC_HIP(hipMemcpyAsync(h->norms + row0, norms_in, (size_t)n * sizeof(float), hipMemcpyDefault, s));
        dispatch_dtype(h->dtype, [&](auto t) { launch_quantize<decltype(t)>(h, nullptr, row0, n, s); });
    });
}

int rc_index_search(rc_index *h, const float *queries, int nq, int64_t n_rows, int k, float *scores, int64_t *out_rows,
                    void *stream) {
    return rc_index_search_ex(h, queries, nq, n_rows, k, scores, out_rows, RC_SEARCH_AUTO, stream);
}

int rc_index_search_ex(rc_index *h, const float *queries, int nq, int64_t n_rows, int k, float *scores,
                       int64_t *out_rows, int mode, void *stream) {
    return rc_index_search_masked(h, queries, nq, n_rows, k, nullptr, scores, out_rows, mode, stream);
}

int rc_index_search_masked(rc_index *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask,
                           float *scores, int64_t *out_rows, int mode, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 256]");
        RC_REQUIRE(n_rows >= 0 && n_rows <= h->capacity, RC_ERR_INVALID, "n_rows out of range");
        RC_REQUIRE(mode == RC_SEARCH_AUTO || mode == RC_SEARCH_SCAN || mode == RC_SEARCH_MFMA || mode == RC_SEARCH_MFMA_MASKED,
                   RC_ERR_INVALID, "unknown search mode");
        // RC_SEARCH_MFMA_MASKED is RC_SEARCH_MFMA (refused where it is, with its errors; the same path
        // without a mask) whose filter kernels read the mask too
        const bool mask_filter = mode == RC_SEARCH_MFMA_MASKED;
        if (mask_filter) mode = RC_SEARCH_MFMA;
        if (nq == 0) return;
        RC_REQUIRE(queries && scores && out_rows, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        hipStream_t s = (hipStream_t)stream;
        // without RC_FILTER_METRIC the batched path's candidate threshold is a bound in cosine space:
        // a non-cosine index scans (AUTO) and refuses MFMA, whatever it holds.  With it the filter
        // bounds the metric's own score (search_mfma.hip) on the f16 / bf16 rows it was set on.
        const bool metric_ok = h->metric == RC_METRIC_COSINE || h->filter == RC_FILTER_METRIC;
        RC_REQUIRE(mode != RC_SEARCH_MFMA || metric_ok, RC_ERR_UNSUPPORTED,
                   "batched MFMA search is cosine-only without RC_FILTER_METRIC (this index scores by dotproduct or euclidean)");
        if (n_rows == 0) {  // an empty shard answers (-inf, -1) in every mode
            empty_search(nq, k, scores, out_rows, s);
            return;
        }
        // (a float8 index scans unless its own filter is switched on: RC_FILTER_F8)
        const bool mfma_ok = metric_ok && ((h->dtype != RC_F32 && h->dtype != RC_F8) || h->rows8 != nullptr ||
                                           h->filter == RC_FILTER_F8);
        RC_REQUIRE(mode != RC_SEARCH_MFMA || mfma_ok, RC_ERR_UNSUPPORTED,
                   "batched MFMA search needs an f16/bf16 index, the int8 filter copy, or a float8 index with RC_FILTER_F8");
        // with a mask AUTO scans: only the caller knows the eligible share, and a selective mask
        // makes the scan cheaper while the filter GEMM still reads every row (MFMA on request)
        bool auto_mfma = nq >= kBatchMinQueries && n_rows >= kBatchMinRows;
        if (h->filter == RC_FILTER_F8) {  // its own corner (see kF8BatchMinPasses)
            const int qb = scan_max_qb(h->nch, k);
            const int passes = (nq + qb - 1) / qb;
            auto_mfma = (passes >= kF8BatchMinPasses && n_rows >= kF8BatchMinRows) ||
                        (passes >= kF8BatchMinPassesLarge && n_rows * h->ld >= kF8BatchMinBytesLarge);
        }
        if (h->filter == RC_FILTER_METRIC && h->metric != RC_METRIC_COSINE)  // its own corner (see kMetricBatchMinQueries); f16 / bf16 rows
            auto_mfma = (nq >= kMetricBatchMinQueries && n_rows >= kBatchMinRows) ||
                        (nq >= kMetricBatchMinQueriesLarge && n_rows * h->ld * 2 >= kMetricBatchMinBytesLarge);
        const bool use_mfma = mode == RC_SEARCH_MFMA || (mode == RC_SEARCH_AUTO && mask == nullptr && mfma_ok && auto_mfma);
        if (!use_mfma) {
            scan_search(h, queries, nq, n_rows, k, mask, scores, out_rows, s);
            return;
        }
        batched_search_exact(h, queries, nq, n_rows, k, mask, mask_filter, scores, out_rows, s);
    });
}

int rc_index_pages_set(rc_index *h, int slot, const int32_t *pages_host, int n_pages, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(slot >= 0 && slot < RC_PAGE_SLOTS_MAX, RC_ERR_INVALID, "slot must be in [0, RC_PAGE_SLOTS_MAX)");
        RC_REQUIRE(n_pages >= 0, RC_ERR_INVALID, "negative page count");
        RC_REQUIRE(n_pages == 0 || pages_host != nullptr, RC_ERR_INVALID, "null page list");
        std::lock_guard<std::mutex> lk(h->mu);
        const int64_t limit = h->capacity / RC_PAGE_ROWS;  // whole pages inside the rows and the norms
        for (int i = 0; i < n_pages; ++i)
            RC_REQUIRE(pages_host[i] >= 0 && pages_host[i] < limit, RC_ERR_INVALID, "page at or past capacity / RC_PAGE_ROWS");
        if (n_pages == 0 && slot >= (int)h->tables.size()) return;
        DeviceScope ds(h->device);
        hipStream_t s = (hipStream_t)stream;
        RC_HIP(hipDeviceSynchronize());  // no search may still read the table
        if (slot >= (int)h->tables.size()) h->tables.resize((size_t)slot + 1);
        rc_index::PageTable &t = h->tables[slot];
        if (n_pages == 0) {
            dfree(t.dev);
            t = rc_index::PageTable{};
            return;
        }
        if (n_pages > t.cap) {
            const int cap2 = std::max(std::max(16, n_pages), 2 * t.cap);
            int32_t *dev = (int32_t *)dmalloc((size_t)cap2 * sizeof(int32_t));
            dfree(t.dev);
            t.dev = dev;
            t.cap = cap2;
            t.n_pages = 0;
        }
        RC_HIP(hipMemcpyAsync(t.dev, pages_host, (size_t)n_pages * sizeof(int32_t), hipMemcpyHostToDevice, s));
        RC_HIP(hipStreamSynchronize(s));  // the host list may be reused; later searches on any stream see the table
        t.n_pages = n_pages;
    });
}

int rc_index_search_pages(rc_index *h, const float *queries, int nq, int slot, int64_t n_pos, int k, const uint32_t *mask,
                          float *scores, int64_t *out_rows, void *stream) {
    return rc_index_search_pages_ex(h, queries, nq, slot, n_pos, k, mask, scores, out_rows, RC_SEARCH_SCAN, stream);
}

int rc_index_search_pages_ex(rc_index *h, const float *queries, int nq, int slot, int64_t n_pos, int k, const uint32_t *mask,
                             float *scores, int64_t *out_rows, int mode, void *stream) {
    return guard([&] {
        RC_REQUIRE(mode == RC_SEARCH_AUTO || mode == RC_SEARCH_SCAN || mode == RC_SEARCH_MFMA || mode == RC_SEARCH_MFMA_MASKED,
                   RC_ERR_INVALID, "unknown search mode");
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 256]");
        RC_REQUIRE(nq == 0 || (queries && scores && out_rows), RC_ERR_INVALID, "null buffer");
        const bool mask_filter = mode == RC_SEARCH_MFMA_MASKED;  // without a mask it is RC_SEARCH_MFMA
        if (mask_filter) mode = RC_SEARCH_MFMA;
        std::lock_guard<std::mutex> lk(h->mu);
        const rc_index::PageTable &t = page_table(h, slot);
        RC_REQUIRE(n_pos >= 0 && n_pos <= (int64_t)t.n_pages * RC_PAGE_ROWS, RC_ERR_INVALID, "n_pos beyond the slot's pages");
        if (nq == 0) return;
        // refused where rc_index_search_ex refuses the mode, and on the int8 and float8 filters, which
        // have no paged form: the paged kernels are the native f16 / bf16 ones, cosine or RC_FILTER_METRIC
        const bool metric_ok = h->metric == RC_METRIC_COSINE || h->filter == RC_FILTER_METRIC;
        RC_REQUIRE(mode != RC_SEARCH_MFMA || metric_ok, RC_ERR_UNSUPPORTED,
                   "batched MFMA search is cosine-only without RC_FILTER_METRIC (this index scores by dotproduct or euclidean)");
        const bool mfma_ok = metric_ok && (h->dtype == RC_F16 || h->dtype == RC_BF16) && h->rows8 == nullptr &&
                             (h->filter == RC_FILTER_NATIVE || h->filter == RC_FILTER_METRIC);
        RC_REQUIRE(mode != RC_SEARCH_MFMA || mfma_ok, RC_ERR_UNSUPPORTED,
                   "batched MFMA search over pages needs an f16/bf16 index with the native or the metric filter");
        RC_REQUIRE(mode != RC_SEARCH_MFMA || paged_filter_supported(h->ld, h->metric != RC_METRIC_COSINE, mask_filter && mask != nullptr),
                   RC_ERR_UNSUPPORTED,
                   "RC_SEARCH_MFMA_MASKED over pages is not available under a non-cosine metric at row width 512 (use RC_SEARCH_MFMA)");
        DeviceScope ds(h->device);
        hipStream_t s = (hipStream_t)stream;
        if (n_pos == 0) {  // this shard holds none of the slot's positions
            empty_search(nq, k, scores, out_rows, s);
            return;
        }
        // with a mask AUTO scans (as rc_index_search_masked, and the masked paged forms are unmeasured)
        const bool auto_mfma = (nq >= kPagedBatchMinQueries && n_pos >= kPagedBatchMinPositions) ||
                               (nq >= kPagedBatchMinQueriesLarge && n_pos >= kPagedBatchMinPositionsLarge);
        const bool use_mfma = mode == RC_SEARCH_MFMA || (mode == RC_SEARCH_AUTO && mask == nullptr && mfma_ok && auto_mfma);
        if (!use_mfma) {
            scan_search(h, queries, nq, n_pos, k, mask, scores, out_rows, s, t.dev);
            return;
        }
        batched_search_exact(h, queries, nq, n_pos, k, mask, mask_filter, scores, out_rows, s, t.dev);
    });
}

int rc_index_search_deep(rc_index *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask, float *scores,
                         int64_t *out_rows, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_DEEP_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 10000]");
        RC_REQUIRE(n_rows >= 0 && n_rows <= h->capacity, RC_ERR_INVALID, "n_rows out of range");
        if (nq == 0) return;
        RC_REQUIRE(queries && scores && out_rows, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        deep_search_locked(h, queries, nq, n_rows, k, mask, nullptr, nullptr, scores, out_rows, (hipStream_t)stream);
    });
}

int rc_index_search_pages_deep(rc_index *h, const float *queries, int nq, int slot, int64_t n_pos, int k, const uint32_t *mask,
                               float *scores, int64_t *out_rows, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_DEEP_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 10000]");
        RC_REQUIRE(nq == 0 || (queries && scores && out_rows), RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        const rc_index::PageTable &t = page_table(h, slot);
        RC_REQUIRE(n_pos >= 0 && n_pos <= (int64_t)t.n_pages * RC_PAGE_ROWS, RC_ERR_INVALID, "n_pos beyond the slot's pages");
        if (nq == 0) return;
        DeviceScope ds(h->device);
        deep_search_locked(h, queries, nq, n_pos, k, mask, t.dev, nullptr, scores, out_rows, (hipStream_t)stream);
    });
}

int rc_index_scores(rc_index *h, const float *query, int64_t n_rows, float *out_scores, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(n_rows >= 0 && n_rows <= h->capacity, RC_ERR_INVALID, "n_rows out of range");
        if (n_rows == 0) return;
        RC_REQUIRE(query && out_scores, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        deep_score_pass(h, query, 1, n_rows, nullptr, out_scores, (hipStream_t)stream);
    });
}

int rc_index_scores_pages(rc_index *h, const float *query, int slot, int64_t n_pos, float *out_scores, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(n_pos == 0 || (query && out_scores), RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        const rc_index::PageTable &t = page_table(h, slot);
        RC_REQUIRE(n_pos >= 0 && n_pos <= (int64_t)t.n_pages * RC_PAGE_ROWS, RC_ERR_INVALID, "n_pos beyond the slot's pages");
        if (n_pos == 0) return;
        DeviceScope ds(h->device);
        deep_score_pass(h, query, 1, n_pos, t.dev, out_scores, (hipStream_t)stream);
    });
}

int rc_index_sparse_enable(rc_index *h, int width, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(width >= 1 && width <= RC_SPARSE_MAX_NNZ, RC_ERR_INVALID, "sparse width must be in [1, 1024]");
        std::lock_guard<std::mutex> lk(h->mu);
        RC_REQUIRE(h->sparse.width == 0 || h->sparse.width == width, RC_ERR_INVALID, "the sparse store has another width already");
        if (h->sparse.width == width) return;
        DeviceScope ds(h->device);
        hipStream_t s = (hipStream_t)stream;
        const size_t slots = (size_t)width * h->capacity;
        uint32_t *idx = (uint32_t *)dmalloc(slots * sizeof(uint32_t));
        float *val = nullptr;
        try {
            val = (float *)dmalloc(slots * sizeof(float));
            RC_HIP(hipMemsetAsync(idx, 0xff, slots * sizeof(uint32_t), s));  // SPARSE_PAD everywhere
            RC_HIP(hipMemsetAsync(val, 0, slots * sizeof(float), s));
            RC_HIP(hipStreamSynchronize(s));
        } catch (...) {
            dfree(idx);
            dfree(val);
            throw;
        }
        h->sparse.idx = idx;
        h->sparse.val = val;
        h->sparse.width = width;
    });
}

int rc_index_sparse_width(const rc_index *h, int *width) {
    return guard([&] {
        RC_REQUIRE(h && width, RC_ERR_INVALID, "null argument");
        *width = h->sparse.width;
    });
}

int rc_index_sparse_write(rc_index *h, const int64_t *rows, const int64_t *off, const uint32_t *idx, const float *val, int64_t n,
                          void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(n >= 0, RC_ERR_INVALID, "negative count");
        if (n == 0) return;
        RC_REQUIRE(rows && off, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        const int width = h->sparse.width;
        RC_REQUIRE(width > 0, RC_ERR_INVALID, "this index has no sparse store (rc_index_sparse_enable)");
        RC_REQUIRE(off[0] == 0, RC_ERR_INVALID, "sparse offsets must start at 0");
        for (int64_t i = 0; i < n; ++i) {
            RC_REQUIRE(rows[i] >= 0 && rows[i] < h->capacity, RC_ERR_INVALID, "row out of capacity");
            const int64_t b = off[i], e = off[i + 1];
            RC_REQUIRE(e >= b && e - b <= width, RC_ERR_INVALID, "a row holds at most the store's width of sparse entries");
            RC_REQUIRE(e == b || (idx && val), RC_ERR_INVALID, "null buffer");
            for (int64_t j = b; j < e; ++j) {
                RC_REQUIRE(idx[j] != SPARSE_PAD, RC_ERR_INVALID, "sparse index 2^32 - 1 is reserved (the store's padding)");
                RC_REQUIRE(j == b || idx[j] > idx[j - 1], RC_ERR_INVALID, "a row's sparse indices must be strictly ascending");
                RC_REQUIRE(std::isfinite(val[j]), RC_ERR_INVALID, "sparse values must be finite");
            }
        }
        DeviceScope ds(h->device);
        hipStream_t s = (hipStream_t)stream;
        // rounds of at most kSparseWriteSlots slots: the staging is sized by the round, not by the call
        const int64_t round = std::max<int64_t>(1, std::min<int64_t>(n, kSparseWriteSlots / width));
        h->sws.ensure_write(round, width);
        SparseWs &w = h->sws;
        for (int64_t r0 = 0; r0 < n; r0 += round) {
            const int64_t m = std::min(round, n - r0);
            w.wait();
            for (int64_t i = 0; i < m; ++i) {
                w.wrow_h[i] = rows[r0 + i];
                const int64_t b = off[r0 + i], cnt = off[r0 + i + 1] - b;
                for (int64_t j = 0; j < width; ++j) {
                    w.widx_h[i * width + j] = j < cnt ? idx[b + j] : SPARSE_PAD;
                    w.wval_h[i * width + j] = j < cnt ? val[b + j] : 0.0f;
                }
            }
            RC_HIP(hipMemcpyAsync(w.wrow_d, w.wrow_h, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, s));
            RC_HIP(hipMemcpyAsync(w.widx_d, w.widx_h, (size_t)m * width * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            RC_HIP(hipMemcpyAsync(w.wval_d, w.wval_h, (size_t)m * width * sizeof(float), hipMemcpyHostToDevice, s));
            RC_HIP(hipEventRecord(w.ev, s));
            w.pending = true;
            launch_sparse_scatter(h->sparse, h->capacity, w.wrow_d, w.widx_d, w.wval_d, m, s);
        }
        RC_HIP(hipStreamSynchronize(s));  // synchronous, as the sharded write: the caller's lists are free and the store is written
        w.pending = false;
    });
}

int rc_index_search_hybrid(rc_index *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask,
                           const int32_t *sq_off, const uint32_t *sq_idx, const float *sq_val, float *scores, int64_t *out_rows,
                           void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_DEEP_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 10000]");
        RC_REQUIRE(n_rows >= 0 && n_rows <= h->capacity, RC_ERR_INVALID, "n_rows out of range");
        if (nq == 0) return;
        RC_REQUIRE(queries && scores && out_rows, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        const SparseQueries sq{sq_off, sq_idx, sq_val};
        check_hybrid(h, sq, nq);
        DeviceScope ds(h->device);
        hipStream_t s = (hipStream_t)stream;
        const DeepAfterScores step = sparse_step(h, sq, nq, n_rows, nullptr, s);
        deep_search_locked(h, queries, nq, n_rows, k, mask, nullptr, nullptr, scores, out_rows, s, step ? &step : nullptr);
    });
}

int rc_index_search_pages_hybrid(rc_index *h, const float *queries, int nq, int slot, int64_t n_pos, int k, const uint32_t *mask,
                                 const int32_t *sq_off, const uint32_t *sq_idx, const float *sq_val, float *scores,
                                 int64_t *out_rows, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_DEEP_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 10000]");
        RC_REQUIRE(nq == 0 || (queries && scores && out_rows), RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        const rc_index::PageTable &t = page_table(h, slot);
        RC_REQUIRE(n_pos >= 0 && n_pos <= (int64_t)t.n_pages * RC_PAGE_ROWS, RC_ERR_INVALID, "n_pos beyond the slot's pages");
        if (nq == 0) return;
        const SparseQueries sq{sq_off, sq_idx, sq_val};
        check_hybrid(h, sq, nq);
        DeviceScope ds(h->device);
        hipStream_t s = (hipStream_t)stream;
        const DeepAfterScores step = sparse_step(h, sq, nq, n_pos, t.dev, s);
        deep_search_locked(h, queries, nq, n_pos, k, mask, t.dev, nullptr, scores, out_rows, s, step ? &step : nullptr);
    });
}

int rc_index_scores_hybrid(rc_index *h, const float *query, int slot, int64_t n, const int32_t *sq_off, const uint32_t *sq_idx,
                           const float *sq_val, float *out_scores, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(n == 0 || (query && out_scores), RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        const int32_t *pages = nullptr;
        if (slot >= 0) {
            const rc_index::PageTable &t = page_table(h, slot);
            RC_REQUIRE(n >= 0 && n <= (int64_t)t.n_pages * RC_PAGE_ROWS, RC_ERR_INVALID, "n_pos beyond the slot's pages");
            pages = t.dev;
        } else {
            RC_REQUIRE(n >= 0 && n <= h->capacity, RC_ERR_INVALID, "n_rows out of range");
        }
        const SparseQueries sq{sq_off, sq_idx, sq_val};
        check_hybrid(h, sq, 1);
        if (n == 0) return;
        DeviceScope ds(h->device);
        hipStream_t s = (hipStream_t)stream;
        const DeepAfterScores step = sparse_step(h, sq, 1, n, pages, s);
        deep_score_pass(h, query, 1, n, pages, out_scores, s);
        if (step) step(0, 1, out_scores, s);
    });
}

int rc_index_filter_scores(rc_index *h, const float *queries, int nq, int64_t row0, int64_t n, float *out_scores,
                           float *out_eps, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0 && n >= 0, RC_ERR_INVALID, "negative count");
        RC_REQUIRE(row0 >= 0 && row0 % 128 == 0 && row0 + n <= h->capacity, RC_ERR_INVALID,
                   "row0 must be a multiple of 128 and the rows inside the capacity");
        if (nq == 0 || n == 0) return;
        RC_REQUIRE(queries && out_scores && out_eps, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        RC_REQUIRE(h->filter == RC_FILTER_F8, RC_ERR_UNSUPPORTED, "filter scores are the float8 filter's (RC_FILTER_F8)");
        DeviceScope ds(h->device);
        h->bws.ensure(nq, 16, h->ld, batch_query_bytes(h));
        BatchPlan p{h->rows, h->dtype, h->dim, h->nch, h->ld, row0 + n, h->row_base, h->row_stride, queries, nq, 16, nullptr, nullptr};
        p.f8_filter = true;
        filter_scores_f8(p, h->bws, row0, n, out_scores, out_eps, (hipStream_t)stream);
    });
}

int rc_topk_merge(const float *scores, const int64_t *rows, int nlists, int nq, int k_in, int k, float *out_scores,
                  int64_t *out_rows, void *stream) {
    return guard([&] {
        RC_REQUIRE(nlists >= 1 && nq >= 0 && k_in >= 1 && k >= 1 && k <= RC_TOPK_MAX, RC_ERR_INVALID, "bad merge sizes");
        if (nq == 0) return;
        hipStream_t s = (hipStream_t)stream;
        with_topk_cap(topk_cap(k), [&](auto cap) {
            hipLaunchKernelGGL(merge_lists_kernel<decltype(cap)::value>, dim3(nq), dim3(256), 0, s, scores, rows, nlists, nq, k_in,
                               k, out_scores, out_rows);
        });
        RC_LAUNCH_CHECK();
    });
}

int rc_index_timing(rc_index *h, int enable) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        if (enable) {
            h->timer.create();
            h->gtimer.create();
        }
        h->timer.enabled = enable != 0;
        h->gtimer.enabled = enable != 0;
    });
}

int rc_index_timing_read(rc_index *h, double *total_ms, int64_t *launches, double *bytes) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        h->timer.flush();
        if (total_ms) *total_ms = h->timer.total_ms;
        if (launches) *launches = h->timer.launches;
        if (bytes) *bytes = h->timer.work;
        h->timer.total_ms = 0;
        h->timer.launches = 0;
        h->timer.work = 0;
    });
}

int rc_index_gemm_timing_read(rc_index *h, double *total_ms, int64_t *launches, double *flops, int64_t *fallbacks) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceScope ds(h->device);
        h->gtimer.flush();
        if (total_ms) *total_ms = h->gtimer.total_ms;
        if (launches) *launches = h->gtimer.launches;
        if (flops) *flops = h->gtimer.work;
        if (fallbacks) {
            int ovf = 0;
            if (h->bws.ovf) {
                RC_HIP(hipDeviceSynchronize());
                RC_HIP(hipMemcpy(&ovf, h->bws.ovf, sizeof(int), hipMemcpyDeviceToHost));
                RC_HIP(hipMemset(h->bws.ovf, 0, sizeof(int)));
            }
            *fallbacks = ovf;
        }
        h->gtimer.total_ms = 0;
        h->gtimer.launches = 0;
        h->gtimer.work = 0;
    });
}

}  // extern "C"
