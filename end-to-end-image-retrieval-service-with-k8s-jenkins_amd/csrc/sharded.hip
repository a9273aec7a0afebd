// sharded.hip — one exact cosine index spread over several shards in ONE process
// (rc_index_create(dim, dtype, capacity_per_gpu, n_gpus); §8(e)).
//
// The Pinecone index the reference opens in get_index (ingesting/utils.py:23-38)
// is one logical index whatever its size; here it is n shards, each an rc_index
// on its own GPU (or several on one GPU).  Routing is round-robin on the
// host-assigned global row g: shard g % n holds it as local row g / n, so rows
// fill every shard evenly from the first upsert on.  A shard returns global rows
// directly (rc_index row map: row_base = s, row_stride = n).
//
// query (retriever/utils.py:62-64): the leader stream's query batch is handed to
// every shard's stream (event wait; a peer copy over xGMI when the shard lives
// on another GPU), each shard runs its own scan / MFMA search over its n_local
// rows, its top-k lists land in a leader-side gather buffer (peer copies of
// nq*k*12 B), and merge_lists_kernel (rc_topk_merge) keys candidates by
// (score desc, global row asc) — the same order a single rc_index gives.
// A multi-PROCESS deployment (one process per GPU) uses the same shard row map
// with an RCCL all-gather instead (sharded.py).
#include <atomic>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "deep.h"
#include "sparse.h"
#include "index_common.h"

namespace rc {
void index_upsert_gather(rc_index *h, const float *vecs, const int64_t *src_idx, int64_t n, const int64_t *rows,
                         hipStream_t s);
void index_move_rows(rc_index *from, const int64_t *src_idx, rc_index *to, const int64_t *dst_idx, const RowBlock &stage,
                     int64_t n, hipStream_t s);
bool index_query1(rc_index *h, const float *query, int64_t n_rows, int k, int with_values, float *out_scores,
                  int64_t *out_rows, float *out_values, hipStream_t s, volatile unsigned **done = nullptr,
                  unsigned *seq = nullptr);
void index_fetch_pages(rc_index *h, int slot, int64_t n_pos, const int64_t *pos, int64_t n, float *out, hipStream_t s);
void index_search_deep_keys(rc_index *h, const float *queries, int nq, int64_t n, int k, const uint32_t *mask, int slot,
                            uint64_t *out_keys, hipStream_t s, const SparseQueries *sq = nullptr);

// Wait for query1's completion word instead of the stream: the word is stored after the results
// (system-scope release), so the host can read them the moment it changes, without the
// end-of-kernel signal round trip.  Every 256 polls the stream is queried, so a faulted or
// finished launch ends the wait too (a fault surfaces as the stream's error).
static void spin_until(volatile unsigned *word, unsigned want, hipStream_t s) {
    for (uint32_t it = 1;; ++it) {
        if (*word == want) return;
        if ((it & 255u) == 0u) {
            const hipError_t e = hipStreamQuery(s);
            if (e == hipSuccess) {
                if (*word == want) return;
                RC_HIP(hipStreamSynchronize(s));
                return;
            }
            if (e != hipErrorNotReady) RC_HIP(e);
        }
        __builtin_ia32_pause();
    }
}

// dst[i][:] = src[idx[i]][:] (one wave per row): a remote shard's subset of an upsert
// batch, made contiguous on the leader so only those rows cross xGMI.
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *__restrict__ src, const int64_t *__restrict__ idx,
                                                         int64_t m, int dim, float *__restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;
    const float *s = src + idx[i] * dim;
    float *d = dst + i * dim;
    for (int c = lane; c < dim; c += 64) d[c] = s[c];
}
}

using namespace rc;

struct rc_sharded {
    std::mutex mu;
    int n = 0, dim = 0, dtype = 0;
    int64_t cap = 0;  // rows per shard
    std::vector<int> dev;
    // shard s is driven through the cross-device path (peer copies to / from the leader):
    // dev[s] != dev[0], or every shard s > 0 after rc_sharded_force_remote (a test hook: the
    // 8-GPU code path — gather, peer copies, leader merge — exercised on one GPU)
    std::vector<char> remote;
    std::vector<rc_index *> shard;
    std::vector<hipStream_t> st;
    std::vector<hipEvent_t> ev_done;   // per shard, recorded on st[s]
    std::vector<hipEvent_t> ev_start;  // per shard, recorded on the caller's (leader) stream
    // search buffers
    int nq_cap = 0, k_cap = 0;
    std::vector<float *> q;       // [nq_cap][dim] query copy on a non-leader shard's device
    std::vector<float *> s_loc;   // [nq_cap][k_cap] a non-leader shard's own result
    std::vector<int64_t *> r_loc;
    float *g_s = nullptr;         // leader [n][nq_cap][k_cap] gathered lists
    int64_t *g_r = nullptr;
    // upsert / fetch staging (grown on demand, reused: no allocation in steady state)
    int64_t st_cap = 0;
    std::vector<int64_t *> idx_d;  // [st_cap] source index per shard (on the leader for a remote shard)
    std::vector<int64_t *> row_d;  // [st_cap] local row per shard (on the shard's device)
    std::vector<float *> vec_d;    // [st_cap][dim] a remote shard's subset of the batch, on its device
    std::vector<float *> gat_d;    // [st_cap][dim] that subset gathered on the leader (peer-copy source)
    std::vector<float *> fo_d;     // [st_cap][dim] fetched rows on the shard's device
    std::vector<int64_t *> idx_h;  // [st_cap] pinned host copies of the per-shard lists
    std::vector<int64_t *> row_h;
    std::vector<float *> fo_h;     // [st_cap][dim] pinned host landing of fetched rows
    hipEvent_t ev_gather = nullptr;  // leader stream: the remote subsets are gathered
    // row moves (rc_sharded_move_rows): per shard the local source / destination rows of one
    // round (kMoveRound entries, pinned + device, made on the first move), and the staging
    // blocks of stored rows that cross devices: mv_out on the source, mv_in on the destination
    // (mv_cap rows each, grown on demand up to kMoveRound, reused)
    bool mv_lists = false;
    int64_t mv_cap = 0;
    std::vector<int64_t *> mv_src_h, mv_dst_h, mv_src_d, mv_dst_d;
    std::vector<RowBlock> mv_out, mv_in;
    std::vector<hipEvent_t> ev_pack;  // per shard, on st[s]: its lists are copied and its outgoing rows packed
    // masked search (rc_sharded_search_masked): the caller's global bitmap de-interleaved into one
    // local bitmap per shard (pinned), and its copy on the shard's device; grown on demand
    int64_t mk_cap = 0;                // words per shard
    std::vector<uint32_t *> mk_h;      // [mk_cap] pinned
    std::vector<uint32_t *> mk_d;      // [mk_cap] on the shard's device
    std::vector<hipEvent_t> ev_mask;   // per shard: its bitmap's H2D copy is done (the pinned words are free again)
    // host-in / host-out query (rc_sharded_query_host): its own leader stream, one pinned
    // staging block and one device block, each laid out [queries | scores | rows | values]
    hipStream_t qs = nullptr;
    int64_t qh_bytes = 0;
    uint8_t *qh = nullptr;  // pinned
    uint8_t *qd = nullptr;  // leader device
    // page tables (rc_sharded_pages_set), by slot: the host copy of the list every shard holds
    // on its device (one page number = the same local rows on every shard); empty = no table
    std::vector<std::vector<int32_t>> tables;
    // deep top-k (rc_sharded_search_deep), several shards: a shard s > 0 keeps a query copy and its
    // own k keys per query on its device, the leader the gathered lists [n][dnq_cap x dk_cap
    // entries used as [n][nq][k]] and the workspace of its selection over them
    int dnq_cap = 0;
    int64_t dkeys_cap = 0;              // keys per shard: nq * k of the largest call
    std::vector<float *> dq;            // [dnq_cap][dim]
    std::vector<uint64_t *> dk_loc;     // [dkeys_cap]
    uint64_t *dg_keys = nullptr;        // leader [n][dkeys_cap]
    DeepSel dsel;
};

namespace {

void free_search(rc_sharded *h) {
    for (int s = 0; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        dfree(h->q[s]);
        dfree(h->s_loc[s]);
        dfree(h->r_loc[s]);
        h->q[s] = nullptr;
        h->s_loc[s] = nullptr;
        h->r_loc[s] = nullptr;
    }
    DeviceScope ds(h->dev[0]);
    dfree(h->g_s);
    dfree(h->g_r);
    h->g_s = nullptr;
    h->g_r = nullptr;
    h->nq_cap = h->k_cap = 0;
}

void ensure_search(rc_sharded *h, int nq, int k) {
    if (nq <= h->nq_cap && k <= h->k_cap) return;
    const int nq2 = std::max(nq, h->nq_cap), k2 = std::max(k, h->k_cap);
    free_search(h);
    for (int s = 0; s < h->n; ++s) {
        if (!h->remote[s]) continue;
        DeviceScope ds(h->dev[s]);
        h->q[s] = (float *)dmalloc((size_t)nq2 * h->dim * sizeof(float));
        h->s_loc[s] = (float *)dmalloc((size_t)nq2 * k2 * sizeof(float));
        h->r_loc[s] = (int64_t *)dmalloc((size_t)nq2 * k2 * sizeof(int64_t));
    }
    DeviceScope ds(h->dev[0]);
    h->g_s = (float *)dmalloc((size_t)h->n * nq2 * k2 * sizeof(float));
    h->g_r = (int64_t *)dmalloc((size_t)h->n * nq2 * k2 * sizeof(int64_t));
    h->nq_cap = nq2;
    h->k_cap = k2;
}

void free_deep(rc_sharded *h) {
    for (int s = 0; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        dfree(h->dq[s]);
        dfree(h->dk_loc[s]);
        h->dq[s] = nullptr;
        h->dk_loc[s] = nullptr;
    }
    DeviceScope dl(h->dev[0]);
    dfree(h->dg_keys);
    h->dg_keys = nullptr;
    h->dnq_cap = 0;
    h->dkeys_cap = 0;
}

// Room for a deep search of nq queries x k keys over several shards.  Every shard past the leader
// gets its buffers whether or not it is remote now (rc_sharded_force_remote changes that later).
void ensure_deep(rc_sharded *h, int nq, int k) {
    const int64_t nk = (int64_t)nq * k;
    if (nq <= h->dnq_cap && nk <= h->dkeys_cap) return;
    const int nq2 = std::max(nq, h->dnq_cap);
    const int64_t nk2 = std::max(nk, h->dkeys_cap);
    free_deep(h);
    for (int s = 1; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        h->dq[s] = (float *)dmalloc((size_t)nq2 * h->dim * sizeof(float));
        h->dk_loc[s] = (uint64_t *)dmalloc((size_t)nk2 * sizeof(uint64_t));
    }
    DeviceScope dl(h->dev[0]);
    h->dg_keys = (uint64_t *)dmalloc((size_t)h->n * nk2 * sizeof(uint64_t));
    h->dnq_cap = nq2;
    h->dkeys_cap = nk2;
}

void free_staging(rc_sharded *h) {
    for (int s = 0; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        dfree(h->row_d[s]);
        dfree(h->vec_d[s]);
        dfree(h->fo_d[s]);
        hfree(h->idx_h[s]);
        hfree(h->row_h[s]);
        hfree(h->fo_h[s]);
        h->row_d[s] = nullptr;
        h->vec_d[s] = h->fo_d[s] = h->fo_h[s] = nullptr;
        h->idx_h[s] = h->row_h[s] = nullptr;
    }
    DeviceScope dl(h->dev[0]);
    for (int s = 0; s < h->n; ++s) {
        dfree(h->idx_d[s]);
        dfree(h->gat_d[s]);
        h->idx_d[s] = nullptr;
        h->gat_d[s] = nullptr;
    }
    h->st_cap = 0;
}

// Per shard, room for m rows of one call: index lists (pinned host + device), the
// remote shards' gathered subset (leader) and its landing (shard device), fetch
// buffers.  Grows geometrically, so a steady stream of calls allocates nothing.
void ensure_staging(rc_sharded *h, int64_t m) {
    if (m <= h->st_cap) return;
    const int64_t m2 = std::max<int64_t>(m, 2 * h->st_cap);
    free_staging(h);
    const size_t vb = (size_t)m2 * h->dim * sizeof(float);
    for (int s = 0; s < h->n; ++s) {
        const bool remote = h->remote[s];
        {
            DeviceScope ds(h->dev[s]);
            h->row_d[s] = (int64_t *)dmalloc((size_t)m2 * sizeof(int64_t));
            h->fo_d[s] = (float *)dmalloc(vb);
            if (remote) h->vec_d[s] = (float *)dmalloc(vb);
        }
        DeviceScope dl(h->dev[0]);  // the source index lists are read on the leader (gather / local upsert)
        h->idx_d[s] = (int64_t *)dmalloc((size_t)m2 * sizeof(int64_t));
        if (remote) h->gat_d[s] = (float *)dmalloc(vb);
        h->idx_h[s] = (int64_t *)hmalloc((size_t)m2 * sizeof(int64_t));
        h->row_h[s] = (int64_t *)hmalloc((size_t)m2 * sizeof(int64_t));
        h->fo_h[s] = (float *)hmalloc(vb);
    }
    h->st_cap = m2;
}

// Row moves run in rounds of this many (source, destination) pairs: the lists and the staging
// blocks are sized by it, not by the call (a delete of millions of rows allocates no more).
constexpr int64_t kMoveRound = 16384;

void free_move_blocks(rc_sharded *h) {
    for (int s = 0; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        for (RowBlock *b : {&h->mv_out[s], &h->mv_in[s]}) {
            dfree(b->rows);
            dfree(b->norms);
            *b = RowBlock{};
        }
    }
    h->mv_cap = 0;
}

void free_move(rc_sharded *h) {
    free_move_blocks(h);
    for (int s = 0; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        dfree(h->mv_src_d[s]);
        dfree(h->mv_dst_d[s]);
        hfree(h->mv_src_h[s]);
        hfree(h->mv_dst_h[s]);
        h->mv_src_d[s] = h->mv_dst_d[s] = h->mv_src_h[s] = h->mv_dst_h[s] = nullptr;
        if (h->ev_pack[s]) (void)hipEventDestroy(h->ev_pack[s]);
        h->ev_pack[s] = nullptr;
    }
    h->mv_lists = false;
}

// The lists of one round per shard, once; and staging blocks of at least m rows on every shard
// that stages (callers pass m <= kMoveRound; m = 0: no pair crosses devices).
void ensure_move(rc_sharded *h, int64_t m, size_t row_bytes) {
    if (!h->mv_lists) {
        try {
            for (int s = 0; s < h->n; ++s) {
                DeviceScope ds(h->dev[s]);
                h->mv_src_d[s] = (int64_t *)dmalloc((size_t)kMoveRound * sizeof(int64_t));
                h->mv_dst_d[s] = (int64_t *)dmalloc((size_t)kMoveRound * sizeof(int64_t));
                h->mv_src_h[s] = (int64_t *)hmalloc((size_t)kMoveRound * sizeof(int64_t));
                h->mv_dst_h[s] = (int64_t *)hmalloc((size_t)kMoveRound * sizeof(int64_t));
                RC_HIP(hipEventCreateWithFlags(&h->ev_pack[s], hipEventDisableTiming));
                // stored rows go straight from their source GPU to their destination GPU
                for (int t = 0; t < s; ++t) {
                    if (h->dev[t] == h->dev[s]) continue;
                    if (hipDeviceEnablePeerAccess(h->dev[t], 0) != hipSuccess) (void)hipGetLastError();
                    DeviceScope dt(h->dev[t]);
                    if (hipDeviceEnablePeerAccess(h->dev[s], 0) != hipSuccess) (void)hipGetLastError();
                }
            }
        } catch (...) {
            free_move(h);
            throw;
        }
        h->mv_lists = true;
    }
    if (m <= h->mv_cap) return;
    const int64_t m2 = std::min<int64_t>(kMoveRound, std::max<int64_t>(m, 2 * h->mv_cap));
    free_move_blocks(h);
    try {
        for (int s = 0; s < h->n; ++s) {
            DeviceScope ds(h->dev[s]);
            for (RowBlock *b : {&h->mv_out[s], &h->mv_in[s]}) {
                b->rows = dmalloc((size_t)m2 * row_bytes);
                b->norms = (float *)dmalloc((size_t)m2 * sizeof(float));
                b->cap = m2;
            }
        }
    } catch (...) {
        free_move_blocks(h);
        throw;
    }
    h->mv_cap = m2;
}

// rows of the global range [0, n_rows) that shard s holds
int64_t shard_rows(const rc_sharded *h, int s, int64_t n_rows) { return n_rows > s ? (n_rows - s + h->n - 1) / h->n : 0; }

void free_mask(rc_sharded *h) {
    for (int s = 0; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        if (h->mk_d[s] != nullptr) (void)hipDeviceSynchronize();  // no search may still read the bitmap
        dfree(h->mk_d[s]);
        hfree(h->mk_h[s]);
        h->mk_d[s] = nullptr;
        h->mk_h[s] = nullptr;
    }
    h->mk_cap = 0;
}

// Split the caller's bitmap over global rows [0, n_rows) into the shards' local bitmaps (global
// row g = local row g / n of shard g % n; with one shard a straight copy) and enqueue each
// shard's H2D copy on the shard's own stream, ahead of its wait for the leader (the bitmap
// does not depend on the queries).  A single shard searches on the caller's stream `ls`, which
// is made to wait for the copy.  Bits at or past n_rows are dropped here; the kernels do not
// rely on that.
// Returns with the copies in flight: wait_mask() before the pinned words are reused.
void stage_mask(rc_sharded *h, const uint32_t *mask, int64_t n_rows, hipStream_t ls) {
    const int n = h->n;
    const int64_t words = (n_rows + 31) / 32;
    const int64_t lw_max = std::max<int64_t>(1, (shard_rows(h, 0, n_rows) + 31) / 32);
    if (lw_max > h->mk_cap) {
        const int64_t w2 = std::max<int64_t>(lw_max, 2 * h->mk_cap);
        free_mask(h);
        for (int s = 0; s < n; ++s) {
            DeviceScope ds(h->dev[s]);
            h->mk_d[s] = (uint32_t *)dmalloc((size_t)w2 * sizeof(uint32_t));
            h->mk_h[s] = (uint32_t *)hmalloc((size_t)w2 * sizeof(uint32_t));
        }
        h->mk_cap = w2;
    }
    if (n == 1) {
        std::memcpy(h->mk_h[0], mask, (size_t)words * sizeof(uint32_t));
    } else {
        for (int s = 0; s < n; ++s) std::memset(h->mk_h[s], 0, (size_t)lw_max * sizeof(uint32_t));
        for (int64_t w = 0; w < words; ++w) {
            uint32_t bits = mask[w];
            while (bits) {  // the set bits only: a selective filter costs its eligible count
                const int64_t g = w * 32 + __builtin_ctz(bits);
                bits &= bits - 1;
                if (g >= n_rows) break;
                const int64_t l = g / n;
                h->mk_h[g - l * n][l >> 5] |= 1u << (l & 31);
            }
        }
    }
    for (int s = 0; s < n; ++s) {
        DeviceScope ds(h->dev[s]);
        const int64_t lw = std::max<int64_t>(1, (shard_rows(h, s, n_rows) + 31) / 32);
        RC_HIP(hipMemcpyAsync(h->mk_d[s], h->mk_h[s], (size_t)lw * sizeof(uint32_t), hipMemcpyHostToDevice, h->st[s]));
        RC_HIP(hipEventRecord(h->ev_mask[s], h->st[s]));
    }
    if (n == 1) RC_HIP(hipStreamWaitEvent(ls, h->ev_mask[0], 0));  // the single shard searches on the caller's stream
}

// Single shard: its search ran on the caller's stream; the shard's own stream (which carries the
// next call's bitmap copy) must not overtake it, whatever stream the next caller brings.
void fence_mask_single(rc_sharded *h, hipStream_t ls) {
    DeviceScope ds(h->dev[0]);
    RC_HIP(hipEventRecord(h->ev_done[0], ls));
    RC_HIP(hipStreamWaitEvent(h->st[0], h->ev_done[0], 0));
}

void wait_mask(rc_sharded *h) {
    for (int s = 0; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        RC_HIP(hipEventSynchronize(h->ev_mask[s]));
    }
}

void free_query(rc_sharded *h) {
    DeviceScope dl(h->dev[0]);
    hfree(h->qh);
    dfree(h->qd);
    h->qh = nullptr;
    h->qd = nullptr;
    h->qh_bytes = 0;
}

// offsets of the query block for nq queries, top-k, with or without values (16-B aligned parts)
struct QueryLayout {
    int64_t q, sc, rw, val, total;
};
QueryLayout query_layout(const rc_sharded *h, int nq, int k, bool values) {
    auto al = [](int64_t b) { return (b + 15) & ~(int64_t)15; };
    QueryLayout L;
    L.q = 0;
    L.sc = al((int64_t)nq * h->dim * 4);
    L.rw = L.sc + al((int64_t)nq * k * 4);
    L.val = L.rw + al((int64_t)nq * k * 8);
    L.total = L.val + (values ? al((int64_t)nq * k * h->dim * 4) : 0);
    return L;
}

void ensure_query(rc_sharded *h, int64_t bytes) {
    if (bytes <= h->qh_bytes) return;
    const int64_t b2 = std::max<int64_t>(bytes, 2 * h->qh_bytes);
    RC_HIP(hipStreamSynchronize(h->qs));
    free_query(h);
    DeviceScope dl(h->dev[0]);
    h->qh = (uint8_t *)hmalloc((size_t)b2);
    h->qd = (uint8_t *)dmalloc((size_t)b2);
    h->qh_bytes = b2;
}

void destroy(rc_sharded *h) {
    free_search(h);
    free_staging(h);
    free_move(h);
    free_mask(h);
    free_deep(h);
    {
        DeviceScope dl(h->dev[0]);
        h->dsel.release();
    }
    if (h->qs) {
        free_query(h);
        DeviceScope dl(h->dev[0]);
        (void)hipStreamDestroy(h->qs);
    }
    for (int s = 0; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        if (h->st[s]) (void)hipStreamDestroy(h->st[s]);
        if (h->ev_done[s]) (void)hipEventDestroy(h->ev_done[s]);
        if (h->ev_start[s]) (void)hipEventDestroy(h->ev_start[s]);
        if (h->ev_mask[s]) (void)hipEventDestroy(h->ev_mask[s]);
        if (h->shard[s]) (void)rc_index_destroy(h->shard[s]);
    }
    if (h->ev_gather) {
        DeviceScope dl(h->dev[0]);
        (void)hipEventDestroy(h->ev_gather);
    }
    delete h;
}

void check_status(int st) {
    if (st != RC_OK) throw Error(st, rc_last_error());
}

}  // namespace

extern "C" {

int rc_sharded_create(int n_shards, const int *devices, int dim, int dtype, int64_t capacity_per_shard, rc_sharded **out) {
    return guard([&] {
        RC_REQUIRE(out && devices, RC_ERR_INVALID, "null argument");
        RC_REQUIRE(n_shards >= 1 && n_shards <= 64, RC_ERR_INVALID, "n_shards must be in [1, 64]");
        RC_REQUIRE(capacity_per_shard > 0 && (double)capacity_per_shard * n_shards < 4294967296.0, RC_ERR_INVALID,
                   "total capacity must be in [1, 2^32) rows (global rows key the cross-shard merge)");
        auto *h = new rc_sharded();
        h->n = n_shards;
        h->dim = dim;
        h->dtype = dtype;
        h->cap = capacity_per_shard;
        h->dev.assign(devices, devices + n_shards);
        h->remote.assign(n_shards, 0);
        for (int s = 1; s < n_shards; ++s) h->remote[s] = devices[s] != devices[0] ? 1 : 0;
        h->shard.assign(n_shards, nullptr);
        h->st.assign(n_shards, nullptr);
        h->ev_done.assign(n_shards, nullptr);
        h->ev_start.assign(n_shards, nullptr);
        h->q.assign(n_shards, nullptr);
        h->s_loc.assign(n_shards, nullptr);
        h->r_loc.assign(n_shards, nullptr);
        h->idx_d.assign(n_shards, nullptr);
        h->row_d.assign(n_shards, nullptr);
        h->vec_d.assign(n_shards, nullptr);
        h->gat_d.assign(n_shards, nullptr);
        h->fo_d.assign(n_shards, nullptr);
        h->idx_h.assign(n_shards, nullptr);
        h->row_h.assign(n_shards, nullptr);
        h->fo_h.assign(n_shards, nullptr);
        h->mv_src_h.assign(n_shards, nullptr);
        h->mv_dst_h.assign(n_shards, nullptr);
        h->mv_src_d.assign(n_shards, nullptr);
        h->mv_dst_d.assign(n_shards, nullptr);
        h->mv_out.assign(n_shards, RowBlock{});
        h->mv_in.assign(n_shards, RowBlock{});
        h->ev_pack.assign(n_shards, nullptr);
        h->mk_h.assign(n_shards, nullptr);
        h->mk_d.assign(n_shards, nullptr);
        h->ev_mask.assign(n_shards, nullptr);
        h->dq.assign(n_shards, nullptr);
        h->dk_loc.assign(n_shards, nullptr);
        try {
            for (int s = 0; s < n_shards; ++s) {
                check_status(rc_index_create(h->dev[s], dim, dtype, capacity_per_shard, s, &h->shard[s]));
                check_status(rc_index_set_row_map(h->shard[s], s, n_shards));
                DeviceScope ds(h->dev[s]);
                RC_HIP(hipStreamCreateWithFlags(&h->st[s], hipStreamNonBlocking));
                RC_HIP(hipEventCreateWithFlags(&h->ev_done[s], hipEventDisableTiming));
                RC_HIP(hipEventCreateWithFlags(&h->ev_mask[s], hipEventDisableTiming));
                if (h->dev[s] != h->dev[0]) {  // direct xGMI peer copies where the platform allows them
                    if (hipDeviceEnablePeerAccess(h->dev[0], 0) != hipSuccess) (void)hipGetLastError();
                    DeviceScope dl(h->dev[0]);
                    if (hipDeviceEnablePeerAccess(h->dev[s], 0) != hipSuccess) (void)hipGetLastError();
                }
            }
            DeviceScope dl(h->dev[0]);
            for (int s = 0; s < n_shards; ++s) RC_HIP(hipEventCreateWithFlags(&h->ev_start[s], hipEventDisableTiming));
            RC_HIP(hipEventCreateWithFlags(&h->ev_gather, hipEventDisableTiming));
            RC_HIP(hipStreamCreateWithFlags(&h->qs, hipStreamNonBlocking));
        } catch (...) {
            destroy(h);
            throw;
        }
        *out = h;
    });
}

int rc_sharded_destroy(rc_sharded *h) {
    return guard([&] {
        if (h) destroy(h);
    });
}

int rc_sharded_force_remote(rc_sharded *h) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        std::lock_guard<std::mutex> lk(h->mu);
        {
            DeviceScope dl(h->dev[0]);
            RC_HIP(hipDeviceSynchronize());  // nothing of the old routing is in flight
        }
        free_search(h);  // both are sized by the remote flags; regrown on the next call
        free_staging(h);
        for (int s = 1; s < h->n; ++s) h->remote[s] = 1;
    });
}

int rc_sharded_info(const rc_sharded *h, int *n_shards, int64_t *capacity_per_shard, int64_t *ld) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        if (n_shards) *n_shards = h->n;
        if (capacity_per_shard) *capacity_per_shard = h->cap;
        if (ld) check_status(rc_index_info(h->shard[0], nullptr, nullptr, nullptr, ld));
    });
}

int rc_sharded_shard(rc_sharded *h, int s, rc_index **out) {
    return guard([&] {
        RC_REQUIRE(h && out, RC_ERR_INVALID, "null argument");
        RC_REQUIRE(s >= 0 && s < h->n, RC_ERR_INVALID, "shard out of range");
        *out = h->shard[s];
    });
}

int rc_sharded_grow(rc_sharded *h, int64_t new_capacity_per_shard) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE((double)new_capacity_per_shard * h->n < 4294967296.0, RC_ERR_INVALID, "total capacity must be < 2^32 rows");
        std::lock_guard<std::mutex> lk(h->mu);
        if (new_capacity_per_shard <= h->cap) return;
        for (int s = 0; s < h->n; ++s) check_status(rc_index_grow(h->shard[s], new_capacity_per_shard, h->st[s]));
        h->cap = new_capacity_per_shard;
    });
}

int rc_sharded_set_filter(rc_sharded *h, int kind) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        std::lock_guard<std::mutex> lk(h->mu);
        // the kind every shard has now (they are set together: shard 0 speaks for all): a refused
        // switch away from RC_FILTER_METRIC (to the int8 or float8 filter under a non-cosine metric)
        // must leave it in place, or the index would lose its batched search.  Only that kind is put
        // back: it allocates nothing, so restoring it cannot fail.  A previous int8 copy was freed by
        // the shards that did switch and is not rebuilt here (it may be what there was no room for):
        // from RC_FILTER_I8 / RC_FILTER_F8 a failure ends at RC_FILTER_NATIVE, as before.
        int prev = RC_FILTER_NATIVE;
        if (h->n > 0) check_status(rc_index_get_filter(h->shard[0], &prev));
        const int back = prev == RC_FILTER_METRIC ? RC_FILTER_METRIC : RC_FILTER_NATIVE;
        try {
            for (int s = 0; s < h->n; ++s) check_status(rc_index_set_filter(h->shard[s], kind, h->st[s]));
        } catch (...) {  // all or nothing: a failed shard (e.g. no room for the int8 copy) rolls every shard back
            for (int s = 0; s < h->n; ++s) (void)rc_index_set_filter(h->shard[s], back, h->st[s]);
            throw;
        }
    });
}

int rc_sharded_set_metric(rc_sharded *h, int metric) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(metric == RC_METRIC_COSINE || metric == RC_METRIC_DOT || metric == RC_METRIC_EUCLIDEAN, RC_ERR_INVALID,
                   "metric must be RC_METRIC_COSINE, RC_METRIC_DOT or RC_METRIC_EUCLIDEAN");
        std::lock_guard<std::mutex> lk(h->mu);
        // validated on every shard before any is set: a refused call leaves one metric everywhere
        for (int s = 0; s < h->n && metric != RC_METRIC_COSINE; ++s) {
            int kind = RC_FILTER_NATIVE;
            check_status(rc_index_get_filter(h->shard[s], &kind));
            RC_REQUIRE(kind == RC_FILTER_NATIVE || kind == RC_FILTER_METRIC, RC_ERR_UNSUPPORTED,
                       "a non-cosine metric on an index with the int8 filter copy or the float8 filter (those filters are cosine-only)");
        }
        for (int s = 0; s < h->n; ++s) check_status(rc_index_set_metric(h->shard[s], metric));
    });
}

int rc_sharded_upsert(rc_sharded *h, const float *vecs, int64_t n, const int64_t *rows, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(n >= 0, RC_ERR_INVALID, "negative count");
        if (n == 0) return;
        RC_REQUIRE(vecs && rows, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        std::vector<int64_t> cnt(h->n, 0);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t g = rows[i];
            RC_REQUIRE(g >= 0 && g / h->n < h->cap, RC_ERR_INVALID, "row out of capacity");
            ++cnt[g % h->n];
        }
        int64_t m = 0;
        for (int s = 0; s < h->n; ++s) m = std::max<int64_t>(m, cnt[s]);
        ensure_staging(h, m);
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int64_t i = 0; i < n; ++i) {  // per-shard (source index, local row) lists, pinned
            const int64_t g = rows[i];
            const int s = (int)(g % h->n);
            h->idx_h[s][cnt[s]] = i;
            h->row_h[s][cnt[s]] = g / h->n;
            ++cnt[s];
        }
        hipStream_t ls = (hipStream_t)stream;
        {
            // leader stream: source lists of every shard, then each remote shard's subset gathered
            // contiguous (cnt[s] rows, not the whole batch, cross xGMI)
            DeviceScope dl(h->dev[0]);
            for (int s = 0; s < h->n; ++s) {
                if (cnt[s] == 0) continue;
                RC_HIP(hipMemcpyAsync(h->idx_d[s], h->idx_h[s], cnt[s] * sizeof(int64_t), hipMemcpyHostToDevice, ls));
                if (h->remote[s]) {
                    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((cnt[s] + 3) / 4)), dim3(256), 0, ls, vecs,
                                       h->idx_d[s], cnt[s], h->dim, h->gat_d[s]);
                    RC_LAUNCH_CHECK();
                }
            }
            RC_HIP(hipEventRecord(h->ev_gather, ls));
        }
        for (int s = 0; s < h->n; ++s) {
            if (cnt[s] == 0) continue;
            DeviceScope ds(h->dev[s]);
            const int64_t ms = cnt[s];
            RC_HIP(hipStreamWaitEvent(h->st[s], h->ev_gather, 0));
            RC_HIP(hipMemcpyAsync(h->row_d[s], h->row_h[s], ms * sizeof(int64_t), hipMemcpyHostToDevice, h->st[s]));
            if (h->remote[s]) {
                RC_HIP(hipMemcpyPeerAsync(h->vec_d[s], h->dev[s], h->gat_d[s], h->dev[0], (size_t)ms * h->dim * sizeof(float),
                                          h->st[s]));
                index_upsert_gather(h->shard[s], h->vec_d[s], nullptr, ms, h->row_d[s], h->st[s]);
            } else {
                index_upsert_gather(h->shard[s], vecs, h->idx_d[s], ms, h->row_d[s], h->st[s]);
            }
        }
        // the pinned lists are reused by the next call: finish here (upsert is synchronous,
        // like the Pinecone call it replaces)
        for (int s = 0; s < h->n; ++s) {
            if (cnt[s] == 0) continue;
            DeviceScope ds(h->dev[s]);
            RC_HIP(hipStreamSynchronize(h->st[s]));
        }
    });
}

int rc_sharded_move_rows(rc_sharded *h, const int64_t *src_rows, const int64_t *dst_rows, int64_t n) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(n >= 0, RC_ERR_INVALID, "negative count");
        if (n == 0) return;
        RC_REQUIRE(src_rows && dst_rows, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        const int ns = h->n;
        {  // everything is checked before the first device call: a refused call has moved nothing
            std::vector<int64_t> a(src_rows, src_rows + n), b(dst_rows, dst_rows + n);
            for (int64_t i = 0; i < n; ++i)
                RC_REQUIRE(a[i] >= 0 && a[i] / ns < h->cap && b[i] >= 0 && b[i] / ns < h->cap, RC_ERR_INVALID,
                           "row out of capacity");
            std::sort(a.begin(), a.end());
            std::sort(b.begin(), b.end());
            RC_REQUIRE(std::adjacent_find(a.begin(), a.end()) == a.end(), RC_ERR_INVALID, "a source row occurs twice");
            RC_REQUIRE(std::adjacent_find(b.begin(), b.end()) == b.end(), RC_ERR_INVALID, "a destination row occurs twice");
            for (int64_t i = 0, j = 0; i < n && j < n;) {
                RC_REQUIRE(a[i] != b[j], RC_ERR_INVALID, "a row is both a source and a destination");
                if (a[i] < b[j]) ++i; else ++j;
            }
        }
        int64_t ld = 0;
        check_status(rc_index_info(h->shard[0], nullptr, nullptr, nullptr, &ld));
        const size_t rb = (size_t)ld * dtype_size(h->dtype);
        // a pair (source shard a, destination shard b) is staged when its rows cross devices (or
        // after rc_sharded_force_remote, as if they did); two shards of one GPU move directly
        auto staged = [&](int a, int b) { return a != b && (h->dev[a] != h->dev[b] || h->remote[a] || h->remote[b]); };
        // per (a, b): pairs, offset of the segment in a's source list and in b's destination list;
        // in both lists the staged segments come last, so one pack and one unpack launch per shard
        // cover them and a segment's place in the staging block is its offset past the first
        std::vector<int64_t> cnt((size_t)ns * ns), soff((size_t)ns * ns), doff((size_t)ns * ns), cur((size_t)ns * ns);
        std::vector<int64_t> s_tot(ns), s_stg(ns), d_tot(ns), d_stg(ns);  // list lengths, first staged entry
        for (int64_t r0 = 0; r0 < n; r0 += kMoveRound) {
            const int64_t m = std::min<int64_t>(kMoveRound, n - r0);
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int64_t i = r0; i < r0 + m; ++i) ++cnt[(size_t)(src_rows[i] % ns) * ns + dst_rows[i] % ns];
            int64_t need = 0;
            for (int a = 0; a < ns; ++a) {
                int64_t so = 0, dof = 0;
                for (int pass = 0; pass < 2; ++pass) {
                    if (pass == 1) s_stg[a] = so, d_stg[a] = dof;
                    for (int b = 0; b < ns; ++b) {
                        if (staged(a, b) == (pass == 1)) soff[(size_t)a * ns + b] = so, so += cnt[(size_t)a * ns + b];
                        if (staged(b, a) == (pass == 1)) doff[(size_t)b * ns + a] = dof, dof += cnt[(size_t)b * ns + a];
                    }
                }
                s_tot[a] = so;
                d_tot[a] = dof;
                need = std::max(need, std::max(so - s_stg[a], dof - d_stg[a]));
            }
            ensure_move(h, need, rb);
            std::fill(cur.begin(), cur.end(), 0);
            for (int64_t i = r0; i < r0 + m; ++i) {
                const int64_t gs = src_rows[i], gd = dst_rows[i];
                const int a = (int)(gs % ns), b = (int)(gd % ns);
                const size_t ab = (size_t)a * ns + b;
                const int64_t k = cur[ab]++;
                h->mv_src_h[a][soff[ab] + k] = gs / ns;
                h->mv_dst_h[b][doff[ab] + k] = gd / ns;
            }
            // Sources and destinations never overlap (validated above; Index.delete's sources are
            // rows at or past the new length, its destinations rows below it), so no row is read
            // after it was written or written twice: the packs, the copies and the unpacks need no
            // order among themselves beyond each pair's own chain (lists -> pack -> copy -> unpack).
            for (int a = 0; a < ns; ++a) {  // each shard's stream: its lists, its own pairs, its pack
                if (s_tot[a] == 0 && d_tot[a] == 0) continue;
                DeviceScope ds(h->dev[a]);
                hipStream_t sa = h->st[a];
                if (s_tot[a])
                    RC_HIP(hipMemcpyAsync(h->mv_src_d[a], h->mv_src_h[a], s_tot[a] * sizeof(int64_t), hipMemcpyHostToDevice, sa));
                if (d_tot[a])
                    RC_HIP(hipMemcpyAsync(h->mv_dst_d[a], h->mv_dst_h[a], d_tot[a] * sizeof(int64_t), hipMemcpyHostToDevice, sa));
                const size_t aa = (size_t)a * ns + a;
                index_move_rows(h->shard[a], h->mv_src_d[a] + soff[aa], h->shard[a], h->mv_dst_d[a] + doff[aa], RowBlock{},
                                cnt[aa], sa);
                index_move_rows(h->shard[a], h->mv_src_d[a] + s_stg[a], nullptr, nullptr, h->mv_out[a], s_tot[a] - s_stg[a], sa);
                RC_HIP(hipEventRecord(h->ev_pack[a], sa));
            }
            for (int b = 0; b < ns; ++b) {  // each destination's stream: what other shards send it
                if (d_tot[b] == 0) continue;
                DeviceScope ds(h->dev[b]);
                hipStream_t sb = h->st[b];
                for (int a = 0; a < ns; ++a) {
                    const size_t ab = (size_t)a * ns + b;
                    if (a == b || cnt[ab] == 0) continue;
                    RC_HIP(hipStreamWaitEvent(sb, h->ev_pack[a], 0));
                    if (!staged(a, b)) {  // one GPU: a's source list is readable here
                        index_move_rows(h->shard[a], h->mv_src_d[a] + soff[ab], h->shard[b], h->mv_dst_d[b] + doff[ab],
                                        RowBlock{}, cnt[ab], sb);
                        continue;
                    }
                    const int64_t from = soff[ab] - s_stg[a], to = doff[ab] - d_stg[b];
                    RC_HIP(hipMemcpyPeerAsync((uint8_t *)h->mv_in[b].rows + (size_t)to * rb, h->dev[b],
                                              (const uint8_t *)h->mv_out[a].rows + (size_t)from * rb, h->dev[a],
                                              (size_t)cnt[ab] * rb, sb));
                    RC_HIP(hipMemcpyPeerAsync(h->mv_in[b].norms + to, h->dev[b], h->mv_out[a].norms + from, h->dev[a],
                                              (size_t)cnt[ab] * sizeof(float), sb));
                }
                index_move_rows(nullptr, nullptr, h->shard[b], h->mv_dst_d[b] + d_stg[b], h->mv_in[b], d_tot[b] - d_stg[b], sb);
            }
            // the pinned lists and the staging blocks are reused by the next round: finish here
            for (int s = 0; s < ns; ++s) {
                if (s_tot[s] == 0 && d_tot[s] == 0) continue;
                DeviceScope ds(h->dev[s]);
                RC_HIP(hipStreamSynchronize(h->st[s]));
            }
        }
    });
}

}  // extern "C"

namespace {

void query_host_checked(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, int with_values,
                        const uint32_t *mask, float *scores, int64_t *out_rows, float *values, int slot);

// rc_sharded_fetch's body (caller holds h->mu)
void fetch_locked(rc_sharded *h, const int64_t *rows, int64_t n, float *out, int stored) {
        std::vector<int64_t> cnt(h->n, 0);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t g = rows[i];
            RC_REQUIRE(g >= 0 && g / h->n < h->cap, RC_ERR_INVALID, "row out of capacity");
            ++cnt[g % h->n];
        }
        int64_t m = 0;
        for (int s = 0; s < h->n; ++s) m = std::max<int64_t>(m, cnt[s]);
        ensure_staging(h, m);
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t g = rows[i];
            const int s = (int)(g % h->n);
            h->idx_h[s][cnt[s]] = i;  // destination row of out
            h->row_h[s][cnt[s]] = g / h->n;
            ++cnt[s];
        }
        // every shard's fetch and D2H copy in flight at once, one wait at the end
        for (int s = 0; s < h->n; ++s) {
            if (cnt[s] == 0) continue;
            DeviceScope ds(h->dev[s]);
            const int64_t ms = cnt[s];
            RC_HIP(hipMemcpyAsync(h->row_d[s], h->row_h[s], ms * sizeof(int64_t), hipMemcpyHostToDevice, h->st[s]));
            check_status(stored ? rc_index_fetch_stored(h->shard[s], h->row_d[s], ms, h->fo_d[s], h->st[s])
                                : rc_index_fetch(h->shard[s], h->row_d[s], ms, h->fo_d[s], h->st[s]));
            RC_HIP(hipMemcpyAsync(h->fo_h[s], h->fo_d[s], (size_t)ms * h->dim * sizeof(float), hipMemcpyDeviceToHost,
                                  h->st[s]));
        }
        for (int s = 0; s < h->n; ++s) {
            if (cnt[s] == 0) continue;
            DeviceScope ds(h->dev[s]);
            RC_HIP(hipStreamSynchronize(h->st[s]));
            for (int64_t j = 0; j < cnt[s]; ++j)
                std::memcpy(out + h->idx_h[s][j] * h->dim, h->fo_h[s] + j * h->dim, (size_t)h->dim * sizeof(float));
        }
}

// rc_sharded_search's body (caller holds h->mu; device buffers on the leader, stream = leader stream)
// mask (optional): HOST bitmap over the global rows; staged per shard first, and the call then
// returns only once the staged words were copied (the next call may overwrite them).
// slot >= 0 (rc_sharded_search_pages): n_rows, the mask and the returned rows are positions of
// that slot; position i is on shard i % n as its position i / n, exactly as global rows are, so
// the split of the mask, the shards' row maps and the merge are the ones of the dense search.
void search_locked(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, float *scores, int64_t *out_rows,
                   int mode, void *stream, const uint32_t *mask = nullptr, int slot = -1) {
        hipStream_t ls = (hipStream_t)stream;
        const bool masked = mask != nullptr;
        if (masked) stage_mask(h, mask, n_rows, ls);
        auto shard_search = [&](int s, const float *q, int64_t n_local, float *so, int64_t *ro, void *st) {
            const uint32_t *m = masked ? h->mk_d[s] : nullptr;
            return slot >= 0 ? rc_index_search_pages_ex(h->shard[s], q, nq, slot, n_local, k, m, so, ro, mode, st)
                             : rc_index_search_masked(h->shard[s], q, nq, n_local, k, m, so, ro, mode, st);
        };
        if (h->n == 1) {
            check_status(shard_search(0, queries, n_rows, scores, out_rows, stream));
            if (masked) {
                fence_mask_single(h, ls);
                wait_mask(h);
            }
            return;
        }
        ensure_search(h, nq, k);
        const int64_t slice = (int64_t)nq * k;
        {
            DeviceScope dl(h->dev[0]);
            for (int s = 0; s < h->n; ++s) RC_HIP(hipEventRecord(h->ev_start[s], ls));
        }
        for (int s = 0; s < h->n; ++s) {
            DeviceScope ds(h->dev[s]);
            RC_HIP(hipStreamWaitEvent(h->st[s], h->ev_start[s], 0));
            const bool local = !h->remote[s];
            const float *q = queries;
            if (!local) {
                RC_HIP(hipMemcpyPeerAsync(h->q[s], h->dev[s], queries, h->dev[0], (size_t)nq * h->dim * sizeof(float), h->st[s]));
                q = h->q[s];
            }
            float *so = local ? h->g_s + s * slice : h->s_loc[s];
            int64_t *ro = local ? h->g_r + s * slice : h->r_loc[s];
            check_status(shard_search(s, q, shard_rows(h, s, n_rows), so, ro, h->st[s]));
            if (!local) {
                RC_HIP(hipMemcpyPeerAsync(h->g_s + s * slice, h->dev[0], so, h->dev[s], slice * sizeof(float), h->st[s]));
                RC_HIP(hipMemcpyPeerAsync(h->g_r + s * slice, h->dev[0], ro, h->dev[s], slice * sizeof(int64_t), h->st[s]));
            }
            RC_HIP(hipEventRecord(h->ev_done[s], h->st[s]));
        }
        DeviceScope dl(h->dev[0]);
        for (int s = 0; s < h->n; ++s) RC_HIP(hipStreamWaitEvent(ls, h->ev_done[s], 0));
        check_status(rc_topk_merge(h->g_s, h->g_r, h->n, nq, k, k, scores, out_rows, stream));
        if (masked) wait_mask(h);
}

// rc_sharded_search_deep's body (caller holds h->mu; device buffers on the leader, stream = leader
// stream), as search_locked: the mask is a HOST bitmap over the global rows (slot >= 0: positions)
// staged per shard.  Each shard selects its own k keys (global rows) with no traffic per round;
// the leader gathers the n lists and runs the same rounds over those n x k keys.  A key's order
// does not depend on the shard that held the row, so the result is that of one index.
// sq (rc_sharded_search_hybrid, checked by the caller): the sparse queries, which every shard stages on
// its own device and adds to its scores before it selects; null: the deep search.
void search_deep_locked(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, float *scores, int64_t *out_rows,
                        void *stream, const uint32_t *mask, int slot, const SparseQueries *sq = nullptr) {
    hipStream_t ls = (hipStream_t)stream;
    const bool masked = mask != nullptr;
    if (masked) stage_mask(h, mask, n_rows, ls);
    if (h->n == 1) {
        const uint32_t *m = masked ? h->mk_d[0] : nullptr;
        if (sq != nullptr)
            check_status(slot >= 0 ? rc_index_search_pages_hybrid(h->shard[0], queries, nq, slot, n_rows, k, m, sq->off, sq->idx, sq->val,
                                                                  scores, out_rows, stream)
                                   : rc_index_search_hybrid(h->shard[0], queries, nq, n_rows, k, m, sq->off, sq->idx, sq->val, scores,
                                                            out_rows, stream));
        else
            check_status(slot >= 0 ? rc_index_search_pages_deep(h->shard[0], queries, nq, slot, n_rows, k, m, scores, out_rows, stream)
                                   : rc_index_search_deep(h->shard[0], queries, nq, n_rows, k, m, scores, out_rows, stream));
        if (masked) {
            fence_mask_single(h, ls);
            wait_mask(h);
        }
        return;
    }
    ensure_deep(h, nq, k);
    const int64_t slice = (int64_t)nq * k;
    {
        DeviceScope dl(h->dev[0]);
        for (int s = 0; s < h->n; ++s) RC_HIP(hipEventRecord(h->ev_start[s], ls));
    }
    for (int s = 0; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        RC_HIP(hipStreamWaitEvent(h->st[s], h->ev_start[s], 0));
        const bool local = !h->remote[s];
        const float *q = queries;
        if (!local) {
            RC_HIP(hipMemcpyPeerAsync(h->dq[s], h->dev[s], queries, h->dev[0], (size_t)nq * h->dim * sizeof(float), h->st[s]));
            q = h->dq[s];
        }
        uint64_t *ko = local ? h->dg_keys + s * slice : h->dk_loc[s];
        index_search_deep_keys(h->shard[s], q, nq, shard_rows(h, s, n_rows), k, masked ? h->mk_d[s] : nullptr, slot, ko, h->st[s],
                               sq);
        if (!local)
            RC_HIP(hipMemcpyPeerAsync(h->dg_keys + s * slice, h->dev[0], ko, h->dev[s], (size_t)slice * sizeof(uint64_t), h->st[s]));
        RC_HIP(hipEventRecord(h->ev_done[s], h->st[s]));
    }
    DeviceScope dl(h->dev[0]);
    for (int s = 0; s < h->n; ++s) RC_HIP(hipStreamWaitEvent(ls, h->ev_done[s], 0));
    const int qc = deep_chunk_queries(nq, (int64_t)h->n * k);
    h->dsel.ensure(qc, (int64_t)qc * k);
    for (int q0 = 0; q0 < nq; q0 += qc) {
        const int m = std::min(qc, nq - q0);
        DeepStream st;
        st.keys = h->dg_keys;  // list s of query q at [(s * nq + q) * k]
        st.n = (int64_t)h->n * k;
        st.klist = k;
        st.nq_total = nq;
        st.q0 = q0;
        deep_select_rounds(st, h->dsel, m, k, h->dsel.keys, ls);
        deep_emit(h->dsel.keys, (int64_t)m * k, scores + (int64_t)q0 * k, out_rows + (int64_t)q0 * k, ls);
    }
    if (masked) wait_mask(h);
}

// What the sharded hybrid calls check of the store and the sparse queries before any device call
// (caller holds h->mu; the shards are enabled and given their metric together: shard 0 speaks for all).
void check_hybrid(const rc_sharded *h, const SparseQueries &sq, int nq) {
    int width = 0, metric = RC_METRIC_COSINE;
    check_status(rc_index_sparse_width(h->shard[0], &width));
    check_status(rc_index_get_metric(h->shard[0], &metric));
    RC_REQUIRE(width > 0, RC_ERR_INVALID, "this index has no sparse store (rc_sharded_sparse_enable)");
    RC_REQUIRE(metric == RC_METRIC_DOT, RC_ERR_INVALID, "sparse-dense hybrid scores need the dotproduct metric");
    sparse_check_queries(sq, nq);
}

}  // namespace

extern "C" {

int rc_sharded_sparse_enable(rc_sharded *h, int width) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(width >= 1 && width <= RC_SPARSE_MAX_NNZ, RC_ERR_INVALID, "sparse width must be in [1, 1024]");
        std::lock_guard<std::mutex> lk(h->mu);
        for (int s = 0; s < h->n; ++s) check_status(rc_index_sparse_enable(h->shard[s], width, h->st[s]));
    });
}

int rc_sharded_sparse_write(rc_sharded *h, const int64_t *rows, const int64_t *off, const uint32_t *idx, const float *val, int64_t n) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(n >= 0, RC_ERR_INVALID, "negative count");
        if (n == 0) return;
        RC_REQUIRE(rows && off, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        RC_REQUIRE(off[0] == 0, RC_ERR_INVALID, "sparse offsets must start at 0");
        for (int64_t i = 0; i < n; ++i) {
            RC_REQUIRE(rows[i] >= 0 && rows[i] < h->cap * h->n, RC_ERR_INVALID, "row out of capacity");
            RC_REQUIRE(off[i + 1] >= off[i], RC_ERR_INVALID, "sparse offsets must not descend");
            RC_REQUIRE(off[i + 1] == off[i] || (idx && val), RC_ERR_INVALID, "null buffer");
        }
        // global row g = local row g / n of shard g % n: one CSR per shard, which the shard checks and writes
        for (int s = 0; s < h->n; ++s) {
            std::vector<int64_t> lrows, loff{0};
            std::vector<uint32_t> lidx;
            std::vector<float> lval;
            for (int64_t i = 0; i < n; ++i) {
                if (rows[i] % h->n != s) continue;
                lrows.push_back(rows[i] / h->n);
                lidx.insert(lidx.end(), idx + off[i], idx + off[i + 1]);
                lval.insert(lval.end(), val + off[i], val + off[i + 1]);
                loff.push_back((int64_t)lidx.size());
            }
            if (lrows.empty()) continue;
            check_status(rc_index_sparse_write(h->shard[s], lrows.data(), loff.data(), lidx.data(), lval.data(), (int64_t)lrows.size(),
                                               h->st[s]));
        }
    });
}

int rc_sharded_search_hybrid(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask,
                             const int32_t *sq_off, const uint32_t *sq_idx, const float *sq_val, float *scores, int64_t *out_rows,
                             void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_DEEP_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 10000]");
        RC_REQUIRE(n_rows >= 0 && n_rows <= h->cap * h->n, RC_ERR_INVALID, "n_rows out of range");
        if (nq == 0) return;
        RC_REQUIRE(queries && scores && out_rows, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        const SparseQueries sq{sq_off, sq_idx, sq_val};
        check_hybrid(h, sq, nq);
        search_deep_locked(h, queries, nq, n_rows, k, scores, out_rows, stream, mask, -1, &sq);
    });
}

int rc_sharded_search_deep(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask, float *scores,
                           int64_t *out_rows, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_DEEP_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 10000]");
        RC_REQUIRE(n_rows >= 0 && n_rows <= h->cap * h->n, RC_ERR_INVALID, "n_rows out of range");
        if (nq == 0) return;
        RC_REQUIRE(queries && scores && out_rows, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        search_deep_locked(h, queries, nq, n_rows, k, scores, out_rows, stream, mask, -1);
    });
}

int rc_sharded_fetch(rc_sharded *h, const int64_t *rows, int64_t n, float *out, int stored) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(n >= 0, RC_ERR_INVALID, "negative count");
        if (n == 0) return;
        RC_REQUIRE(rows && out, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        fetch_locked(h, rows, n, out, stored);
    });
}

int rc_sharded_search(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, float *scores,
                      int64_t *out_rows, int mode, void *stream) {
    return rc_sharded_search_masked(h, queries, nq, n_rows, k, nullptr, scores, out_rows, mode, stream);
}

int rc_sharded_search_masked(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask,
                             float *scores, int64_t *out_rows, int mode, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 256]");
        RC_REQUIRE(n_rows >= 0 && n_rows <= h->cap * h->n, RC_ERR_INVALID, "n_rows out of range");
        if (nq == 0) return;
        RC_REQUIRE(queries && scores && out_rows, RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        search_locked(h, queries, nq, n_rows, k, scores, out_rows, mode, stream, mask);
    });
}

int rc_sharded_query_host(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, int with_values,
                          float *scores, int64_t *out_rows, float *values) {
    return rc_sharded_query_host_masked(h, queries, nq, n_rows, k, with_values, nullptr, scores, out_rows, values);
}

int rc_sharded_query_host_masked(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, int with_values,
                                 const uint32_t *mask, float *scores, int64_t *out_rows, float *values) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 256]");
        RC_REQUIRE(n_rows >= 0 && n_rows <= h->cap * h->n, RC_ERR_INVALID, "n_rows out of range");
        if (nq == 0) return;
        RC_REQUIRE(queries && scores && out_rows && (!with_values || values), RC_ERR_INVALID, "null buffer");
        query_host_checked(h, queries, nq, n_rows, k, with_values, mask, scores, out_rows, values, -1);
    });
}

}  // extern "C"

namespace {

// The table of a slot and the range of n_pos it covers, or an error (caller holds h->mu).
const std::vector<int32_t> &page_list(const rc_sharded *h, int slot, int64_t n_pos) {
    RC_REQUIRE(slot >= 0 && slot < (int)h->tables.size() && !h->tables[slot].empty(), RC_ERR_INVALID,
               "unknown slot (no page table was set for it)");
    const std::vector<int32_t> &L = h->tables[slot];
    RC_REQUIRE(n_pos >= 0 && n_pos <= (int64_t)L.size() * RC_PAGE_ROWS * h->n, RC_ERR_INVALID, "n_pos beyond the slot's pages");
    return L;
}

// rc_sharded_query_host_masked's body after its argument checks; slot >= 0:
// rc_sharded_query_host_pages (n_rows and out_rows are positions of that slot).
void query_host_checked(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, int with_values,
                        const uint32_t *mask, float *scores, int64_t *out_rows, float *values, int slot) {
        const int64_t nk = (int64_t)nq * k;
        if (n_rows == 0) {  // an empty index: empty lists, no device work
            std::fill(scores, scores + nk, -INFINITY);
            std::fill(out_rows, out_rows + nk, (int64_t)-1);
            return;
        }
        std::lock_guard<std::mutex> lk(h->mu);
        if (slot >= 0) (void)page_list(h, slot, n_rows);  // under the lock, before any device call
        // one shard: the matched rows' values are gathered on the device and come back in the
        // same copy as the lists; several shards: values through the staged fetch afterwards
        const bool dev_values = with_values && h->n == 1;
        const QueryLayout L = query_layout(h, nq, k, dev_values);
        ensure_query(h, L.total);
        DeviceScope dl(h->dev[0]);
        if (slot < 0 && h->n == 1 && nq == 1 && mask == nullptr) {
            // the request path: one launch pair (query in the kernel arguments, results written
            // straight into the pinned block), no copies; the host polls the completion word
            float *hs = (float *)(h->qh + L.sc);
            int64_t *hr = (int64_t *)(h->qh + L.rw);
            float *hv = (float *)(h->qh + L.val);
            volatile unsigned *word = nullptr;
            unsigned want = 0;
            if (index_query1(h->shard[0], queries, n_rows, k, with_values, hs, hr, hv, h->qs, &word, &want)) {
                spin_until(word, want, h->qs);
                std::atomic_thread_fence(std::memory_order_acquire);  // the result reads stay below
                std::memcpy(scores, hs, (size_t)k * sizeof(float));
                std::memcpy(out_rows, hr, (size_t)k * sizeof(int64_t));
                if (with_values) std::memcpy(values, hv, (size_t)k * h->dim * sizeof(float));
                return;
            }
        }
        std::memcpy(h->qh + L.q, queries, (size_t)nq * h->dim * sizeof(float));
        RC_HIP(hipMemcpyAsync(h->qd + L.q, h->qh + L.q, (size_t)nq * h->dim * sizeof(float), hipMemcpyHostToDevice, h->qs));
        float *dsc = (float *)(h->qd + L.sc);
        int64_t *drw = (int64_t *)(h->qd + L.rw);
        search_locked(h, (const float *)(h->qd + L.q), nq, n_rows, k, dsc, drw, slot >= 0 ? RC_SEARCH_SCAN : RC_SEARCH_AUTO, h->qs, mask,
                      slot);  // a slot scans, as before the paged batched search
        if (dev_values) {
            if (slot >= 0) index_fetch_pages(h->shard[0], slot, n_rows, drw, nk, (float *)(h->qd + L.val), h->qs);
            else check_status(rc_index_fetch(h->shard[0], drw, nk, (float *)(h->qd + L.val), h->qs));
        }
        RC_HIP(hipMemcpyAsync(h->qh + L.sc, h->qd + L.sc, (size_t)(L.total - L.sc), hipMemcpyDeviceToHost, h->qs));
        RC_HIP(hipStreamSynchronize(h->qs));
        std::memcpy(scores, h->qh + L.sc, (size_t)nk * sizeof(float));
        std::memcpy(out_rows, h->qh + L.rw, (size_t)nk * sizeof(int64_t));
        if (dev_values) {
            std::memcpy(values, h->qh + L.val, (size_t)nk * h->dim * sizeof(float));
        } else if (with_values) {
            std::vector<int64_t> live;
            std::vector<int64_t> at;
            for (int64_t i = 0; i < nk; ++i)
                if (out_rows[i] >= 0) {
                    int64_t g = out_rows[i];
                    if (slot >= 0) {  // position -> global row through the slot's pages
                        const int64_t span = (int64_t)RC_PAGE_ROWS * h->n;
                        g = (int64_t)h->tables[slot][g / span] * span + g % span;
                    }
                    live.push_back(g);
                    at.push_back(i);
                } else {
                    std::fill(values + i * h->dim, values + (i + 1) * h->dim, NAN);
                }
            if (!live.empty()) {
                std::vector<float> tmp(live.size() * (size_t)h->dim);
                fetch_locked(h, live.data(), (int64_t)live.size(), tmp.data(), 0);
                for (size_t j = 0; j < live.size(); ++j)
                    std::memcpy(values + at[j] * h->dim, tmp.data() + j * h->dim, (size_t)h->dim * sizeof(float));
            }
        }
}

}  // namespace

extern "C" {

int rc_sharded_pages_set(rc_sharded *h, int slot, const int32_t *pages_host, int n_pages) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(slot >= 0 && slot < RC_PAGE_SLOTS_MAX, RC_ERR_INVALID, "slot must be in [0, RC_PAGE_SLOTS_MAX)");
        RC_REQUIRE(n_pages >= 0, RC_ERR_INVALID, "negative page count");
        RC_REQUIRE(n_pages == 0 || pages_host != nullptr, RC_ERR_INVALID, "null page list");
        std::lock_guard<std::mutex> lk(h->mu);
        const int64_t limit = h->cap / RC_PAGE_ROWS;
        for (int i = 0; i < n_pages; ++i)
            RC_REQUIRE(pages_host[i] >= 0 && pages_host[i] < limit, RC_ERR_INVALID,
                       "page at or past capacity_per_shard / RC_PAGE_ROWS");
        if (n_pages == 0 && slot >= (int)h->tables.size()) return;
        if (slot >= (int)h->tables.size()) h->tables.resize((size_t)slot + 1);
        h->tables[slot].clear();  // a failure below leaves the slot unknown, never half installed
        for (int s = 0; s < h->n; ++s) check_status(rc_index_pages_set(h->shard[s], slot, pages_host, n_pages, h->st[s]));
        h->tables[slot].assign(pages_host, pages_host + n_pages);
    });
}

int rc_sharded_search_pages(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k, const uint32_t *mask,
                            float *scores, int64_t *out_rows, void *stream) {
    return rc_sharded_search_pages_ex(h, queries, nq, slot, n_pos, k, mask, scores, out_rows, RC_SEARCH_SCAN, stream);
}

int rc_sharded_search_pages_ex(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k, const uint32_t *mask,
                               float *scores, int64_t *out_rows, int mode, void *stream) {
    return guard([&] {
        RC_REQUIRE(mode == RC_SEARCH_AUTO || mode == RC_SEARCH_SCAN || mode == RC_SEARCH_MFMA || mode == RC_SEARCH_MFMA_MASKED,
                   RC_ERR_INVALID, "unknown search mode");
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 256]");
        RC_REQUIRE(nq == 0 || (queries && scores && out_rows), RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        (void)page_list(h, slot, n_pos);
        if (nq == 0) return;
        search_locked(h, queries, nq, n_pos, k, scores, out_rows, mode, stream, mask, slot);  // every shard takes the mode
    });
}

int rc_sharded_search_pages_deep(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k, const uint32_t *mask,
                                 float *scores, int64_t *out_rows, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_DEEP_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 10000]");
        RC_REQUIRE(nq == 0 || (queries && scores && out_rows), RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        (void)page_list(h, slot, n_pos);
        if (nq == 0) return;
        search_deep_locked(h, queries, nq, n_pos, k, scores, out_rows, stream, mask, slot);
    });
}

int rc_sharded_search_pages_hybrid(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k, const uint32_t *mask,
                                   const int32_t *sq_off, const uint32_t *sq_idx, const float *sq_val, float *scores,
                                   int64_t *out_rows, void *stream) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_DEEP_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 10000]");
        RC_REQUIRE(nq == 0 || (queries && scores && out_rows), RC_ERR_INVALID, "null buffer");
        std::lock_guard<std::mutex> lk(h->mu);
        (void)page_list(h, slot, n_pos);
        if (nq == 0) return;
        const SparseQueries sq{sq_off, sq_idx, sq_val};
        check_hybrid(h, sq, nq);
        search_deep_locked(h, queries, nq, n_pos, k, scores, out_rows, stream, mask, slot, &sq);
    });
}

int rc_sharded_query_host_pages(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k, int with_values,
                                const uint32_t *mask, float *scores, int64_t *out_rows, float *values) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(nq >= 0, RC_ERR_INVALID, "negative query count");
        RC_REQUIRE(k >= 1 && k <= RC_TOPK_MAX, RC_ERR_INVALID, "top_k must be in [1, 256]");
        RC_REQUIRE(nq == 0 || (queries && scores && out_rows && (!with_values || values)), RC_ERR_INVALID, "null buffer");
        RC_REQUIRE(slot >= 0 && slot < RC_PAGE_SLOTS_MAX && n_pos >= 0, RC_ERR_INVALID, "slot or n_pos out of range");
        if (nq == 0 || n_pos == 0) {
            std::lock_guard<std::mutex> lk(h->mu);
            (void)page_list(h, slot, n_pos);
            if (nq == 0) return;
        }
        query_host_checked(h, queries, nq, n_pos, k, with_values, mask, scores, out_rows, values, slot);
    });
}

}  // extern "C"
