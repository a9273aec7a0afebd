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
void index_search_deep(rc_index *h, const float *queries, int nq, int64_t n, int k, const uint32_t *mask, int slot,
                       uint64_t *out_keys, float *scores, int64_t *out_rows, hipStream_t s, const SparseQueries *sq);

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

// The owning form of a RowBlock: the staging blocks of a row move.
struct RowStage {
    DevBuf<void> rows;
    DevBuf<float> norms;
    RowBlock view() const { return RowBlock{rows.get(), norms.get(), (int64_t)norms.capacity()}; }
};

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
    std::vector<DevBuf<float>> q;      // [nq_cap][dim] query copy on a non-leader shard's device
    std::vector<DevBuf<void>> s_loc;   // [nq_cap][k_cap] f32: a non-leader shard's own result
    std::vector<DevBuf<void>> r_loc;   // ... and its int64 rows
    DevBuf<float> g_s;                 // leader [n][nq_cap][k_cap] gathered lists
    DevBuf<int64_t> g_r;
    // upsert / fetch staging for st_cap() rows per shard (grown on demand, reused: no allocation in steady state)
    std::vector<DevBuf<int64_t>> idx_d;  // source index per shard (on the leader for a remote shard)
    std::vector<DevBuf<int64_t>> row_d;  // local row per shard (on the shard's device)
    std::vector<DevBuf<float>> vec_d;    // [..][dim] a remote shard's subset of the batch, on its device
    std::vector<DevBuf<float>> gat_d;    // [..][dim] that subset gathered on the leader (peer-copy source)
    std::vector<DevBuf<float>> fo_d;     // [..][dim] fetched rows on the shard's device
    std::vector<PinBuf<int64_t>> idx_h;  // pinned host copies of the per-shard lists
    std::vector<PinBuf<int64_t>> row_h;
    std::vector<PinBuf<float>> fo_h;     // [..][dim] pinned host landing of fetched rows
    hipEvent_t ev_gather = nullptr;  // leader stream: the remote subsets are gathered
    // row moves (rc_sharded_move_rows): per shard the local source / destination rows of one
    // round (kMoveRound entries, pinned + device, made on the first move), and the staging
    // blocks of stored rows that cross devices: mv_out on the source, mv_in on the destination
    // (mv_cap() rows each, grown on demand up to kMoveRound, reused)
    bool mv_lists = false;
    std::vector<PinBuf<int64_t>> mv_src_h, mv_dst_h;
    std::vector<DevBuf<int64_t>> mv_src_d, mv_dst_d;
    std::vector<RowStage> mv_out, mv_in;
    std::vector<hipEvent_t> ev_pack;  // per shard, on st[s]: its lists are copied and its outgoing rows packed
    // masked search (rc_sharded_search_masked): the caller's global bitmap de-interleaved into one
    // local bitmap per shard (pinned), and its copy on the shard's device; grown on demand
    std::vector<PinBuf<uint32_t>> mk_h;  // pinned, mk_cap() words per shard
    std::vector<DevBuf<uint32_t>> mk_d;  // on the shard's device
    std::vector<hipEvent_t> ev_mask;   // per shard: its bitmap's H2D copy is done (the pinned words are free again)
    // host-in / host-out query (rc_sharded_query_host): its own leader stream, one pinned
    // staging block and one device block, each laid out [queries | scores | rows | values]
    hipStream_t qs = nullptr;
    PinBuf<uint8_t> qh;
    DevBuf<uint8_t> qd;  // leader device
    // page tables (rc_sharded_pages_set), by slot: the host copy of the list every shard holds
    // on its device (one page number = the same local rows on every shard); empty = no table
    std::vector<std::vector<int32_t>> tables;
    // deep top-k (rc_sharded_search_deep), several shards: a shard s > 0 keeps a query copy and its
    // own k keys per query on its device, the leader the gathered lists [n][dkeys_cap()
    // entries used as [n][nq][k]] and the workspace of its selection over them
    int dnq_cap = 0;
    std::vector<DevBuf<float>> dq;      // [dnq_cap][dim]
    std::vector<DevBuf<void>> dk_loc;   // dkeys_cap() uint64 keys: nq * k of the largest call
    DevBuf<uint64_t> dg_keys;           // leader [n][dkeys_cap()]
    DeepSel dsel;
    int deep_select = RC_DEEP_SELECT_ROUNDS;  // the selection of the leader's merge (rc_sharded_set_deep_select)
};

namespace {

// The sizes of the staging groups below are read off the block each group reserves last: every
// ensure_* frees its whole group before it reserves, so that block is there only if all are.
int64_t dkeys_cap(const rc_sharded *h) { return (int64_t)h->dg_keys.capacity() / h->n; }
int64_t st_cap(const rc_sharded *h) { return (int64_t)h->row_h.back().capacity(); }
int64_t mv_cap(const rc_sharded *h) { return (int64_t)h->mv_in.back().norms.capacity(); }
int64_t mk_cap(const rc_sharded *h) { return (int64_t)h->mk_h.back().capacity(); }

void free_search(rc_sharded *h) {
    h->nq_cap = h->k_cap = 0;
    for (int s = 0; s < h->n; ++s) {
        h->q[s].reset();
        h->s_loc[s].reset();
        h->r_loc[s].reset();
    }
    h->g_s.reset();
    h->g_r.reset();
}

void ensure_search(rc_sharded *h, int nq, int k) {
    if (nq <= h->nq_cap && k <= h->k_cap) return;
    const int nq2 = std::max(nq, h->nq_cap), k2 = std::max(k, h->k_cap);
    free_search(h);
    for (int s = 0; s < h->n; ++s) {
        if (!h->remote[s]) continue;
        DeviceScope ds(h->dev[s]);
        h->q[s].reserve((size_t)nq2 * h->dim);
        h->s_loc[s].reserve((size_t)nq2 * k2 * sizeof(float));
        h->r_loc[s].reserve((size_t)nq2 * k2 * sizeof(int64_t));
    }
    DeviceScope ds(h->dev[0]);
    h->g_s.reserve((size_t)h->n * nq2 * k2);
    h->g_r.reserve((size_t)h->n * nq2 * k2);
    h->nq_cap = nq2;
    h->k_cap = k2;
}

// Room for a deep search of nq queries x k keys over several shards.  Every shard past the leader
// gets its buffers whether or not it is remote now (rc_sharded_force_remote changes that later).
void ensure_deep(rc_sharded *h, int nq, int k) {
    const int64_t nk = (int64_t)nq * k;
    if (nq <= h->dnq_cap && nk <= dkeys_cap(h)) return;
    const int nq2 = std::max(nq, h->dnq_cap);
    const int64_t nk2 = std::max(nk, dkeys_cap(h));
    h->dnq_cap = 0;
    h->dg_keys.reset();
    for (int s = 1; s < h->n; ++s) {
        h->dq[s].reset();
        h->dk_loc[s].reset();
    }
    for (int s = 1; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        h->dq[s].reserve((size_t)nq2 * h->dim);
        h->dk_loc[s].reserve((size_t)nk2 * sizeof(uint64_t));
    }
    DeviceScope dl(h->dev[0]);
    h->dg_keys.reserve((size_t)h->n * nk2);
    h->dnq_cap = nq2;
}

void free_staging(rc_sharded *h) {
    for (int s = 0; s < h->n; ++s) {
        h->row_d[s].reset();
        h->vec_d[s].reset();
        h->fo_d[s].reset();
        h->idx_d[s].reset();
        h->gat_d[s].reset();
        h->idx_h[s].reset();
        h->fo_h[s].reset();
        h->row_h[s].reset();
    }
}

// Per shard, room for m rows of one call: index lists (pinned host + device), the
// remote shards' gathered subset (leader) and its landing (shard device), fetch
// buffers.  Grows geometrically, so a steady stream of calls allocates nothing.
void ensure_staging(rc_sharded *h, int64_t m) {
    if (m <= st_cap(h)) return;
    const size_t m2 = (size_t)std::max<int64_t>(m, 2 * st_cap(h));
    free_staging(h);
    const size_t vn = m2 * h->dim;
    for (int s = 0; s < h->n; ++s) {
        const bool remote = h->remote[s];
        {
            DeviceScope ds(h->dev[s]);
            h->row_d[s].reserve(m2);
            h->fo_d[s].reserve(vn);
            if (remote) h->vec_d[s].reserve(vn);
        }
        DeviceScope dl(h->dev[0]);  // the source index lists are read on the leader (gather / local upsert)
        h->idx_d[s].reserve(m2);
        if (remote) h->gat_d[s].reserve(vn);
        h->idx_h[s].reserve(m2);
        h->fo_h[s].reserve(vn);
        h->row_h[s].reserve(m2);
    }
}

// Row moves run in rounds of this many (source, destination) pairs: the lists and the staging
// blocks are sized by it, not by the call (a delete of millions of rows allocates no more).
constexpr int64_t kMoveRound = 16384;

// The lists of one round per shard, once; and staging blocks of at least m rows on every shard
// that stages (callers pass m <= kMoveRound; m = 0: no pair crosses devices).
void ensure_move(rc_sharded *h, int64_t m, size_t row_bytes) {
    if (!h->mv_lists) {  // (a failure part of the way: the next call takes it up from there)
        for (int s = 0; s < h->n; ++s) {
            DeviceScope ds(h->dev[s]);
            h->mv_src_d[s].reserve((size_t)kMoveRound);
            h->mv_dst_d[s].reserve((size_t)kMoveRound);
            h->mv_src_h[s].reserve((size_t)kMoveRound);
            h->mv_dst_h[s].reserve((size_t)kMoveRound);
            if (h->ev_pack[s] == nullptr) RC_HIP(hipEventCreateWithFlags(&h->ev_pack[s], hipEventDisableTiming));
            // stored rows go straight from their source GPU to their destination GPU
            for (int t = 0; t < s; ++t) {
                if (h->dev[t] == h->dev[s]) continue;
                if (hipDeviceEnablePeerAccess(h->dev[t], 0) != hipSuccess) (void)hipGetLastError();
                DeviceScope dt(h->dev[t]);
                if (hipDeviceEnablePeerAccess(h->dev[s], 0) != hipSuccess) (void)hipGetLastError();
            }
        }
        h->mv_lists = true;
    }
    if (m <= mv_cap(h)) return;
    const size_t m2 = (size_t)std::min<int64_t>(kMoveRound, std::max<int64_t>(m, 2 * mv_cap(h)));
    for (int s = 0; s < h->n; ++s) {
        h->mv_out[s] = RowStage{};
        h->mv_in[s] = RowStage{};
    }
    for (int s = 0; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        for (RowStage *b : {&h->mv_out[s], &h->mv_in[s]}) {
            b->rows.reserve(m2 * row_bytes);
            b->norms.reserve(m2);
        }
    }
}

// rows of the global range [0, n_rows) that shard s holds
int64_t shard_rows(const rc_sharded *h, int s, int64_t n_rows) { return n_rows > s ? (n_rows - s + h->n - 1) / h->n : 0; }

void free_mask(rc_sharded *h) {
    for (int s = 0; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        if (!h->mk_d[s].empty()) (void)hipDeviceSynchronize();  // no search may still read the bitmap
        h->mk_d[s].reset();
        h->mk_h[s].reset();
    }
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
    if (lw_max > mk_cap(h)) {
        const size_t w2 = (size_t)std::max<int64_t>(lw_max, 2 * mk_cap(h));
        free_mask(h);
        for (int s = 0; s < n; ++s) {
            DeviceScope ds(h->dev[s]);
            h->mk_d[s].reserve(w2);
            h->mk_h[s].reserve(w2);
        }
    }
    if (n == 1) {
        std::memcpy(h->mk_h[0].get(), mask, (size_t)words * sizeof(uint32_t));
    } else {
        for (int s = 0; s < n; ++s) std::memset(h->mk_h[s].get(), 0, (size_t)lw_max * sizeof(uint32_t));
        for (int64_t w = 0; w < words; ++w) {
            uint32_t bits = mask[w];
            while (bits) {  // the set bits only: a selective filter costs its eligible count
                const int64_t g = w * 32 + __builtin_ctz(bits);
                bits &= bits - 1;
                if (g >= n_rows) break;
                const int64_t l = g / n;
                h->mk_h[g - l * n].get()[l >> 5] |= 1u << (l & 31);
            }
        }
    }
    for (int s = 0; s < n; ++s) {
        DeviceScope ds(h->dev[s]);
        const int64_t lw = std::max<int64_t>(1, (shard_rows(h, s, n_rows) + 31) / 32);
        RC_HIP(hipMemcpyAsync(h->mk_d[s].get(), h->mk_h[s].get(), (size_t)lw * sizeof(uint32_t), hipMemcpyHostToDevice, h->st[s]));
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
    if ((size_t)bytes <= min_capacity(h->qh, h->qd)) return;
    const size_t b2 = std::max<size_t>(bytes, 2 * min_capacity(h->qh, h->qd));
    RC_HIP(hipStreamSynchronize(h->qs));
    DeviceScope dl(h->dev[0]);
    h->qh.reserve(b2);
    h->qd.reserve(b2);
}

void destroy(rc_sharded *h) {
    free_mask(h);  // (waits for the searches that read the bitmaps)
    if (h->qs) {
        DeviceScope dl(h->dev[0]);
        (void)hipStreamDestroy(h->qs);
    }
    for (int s = 0; s < h->n; ++s) {
        DeviceScope ds(h->dev[s]);
        if (h->st[s]) (void)hipStreamDestroy(h->st[s]);
        if (h->ev_done[s]) (void)hipEventDestroy(h->ev_done[s]);
        if (h->ev_start[s]) (void)hipEventDestroy(h->ev_start[s]);
        if (h->ev_mask[s]) (void)hipEventDestroy(h->ev_mask[s]);
        if (h->ev_pack[s]) (void)hipEventDestroy(h->ev_pack[s]);
        if (h->shard[s]) (void)rc_index_destroy(h->shard[s]);
    }
    if (h->ev_gather) {
        DeviceScope dl(h->dev[0]);
        (void)hipEventDestroy(h->ev_gather);
    }
    delete h;  // the buffers free themselves
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
        for (auto *v : {&h->q, &h->vec_d, &h->gat_d, &h->fo_d, &h->dq}) v->resize(n_shards);
        for (auto *v : {&h->s_loc, &h->r_loc, &h->dk_loc}) v->resize(n_shards);
        for (auto *v : {&h->idx_d, &h->row_d, &h->mv_src_d, &h->mv_dst_d}) v->resize(n_shards);
        for (auto *v : {&h->idx_h, &h->row_h, &h->mv_src_h, &h->mv_dst_h}) v->resize(n_shards);
        h->fo_h.resize(n_shards);
        h->mv_out.resize(n_shards);
        h->mv_in.resize(n_shards);
        h->ev_pack.assign(n_shards, nullptr);
        h->mk_h.resize(n_shards);
        h->mk_d.resize(n_shards);
        h->ev_mask.assign(n_shards, nullptr);
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
        // (RC_FILTER_F32 likewise: it too allocates nothing and carries a non-cosine index's batched search)
        const int back = prev == RC_FILTER_METRIC || prev == RC_FILTER_F32 ? prev : RC_FILTER_NATIVE;
        try {
            for (int s = 0; s < h->n; ++s) check_status(rc_index_set_filter(h->shard[s], kind, h->st[s]));
        } catch (...) {  // all or nothing: a failed shard (e.g. no room for the int8 copy) rolls every shard back
            for (int s = 0; s < h->n; ++s) (void)rc_index_set_filter(h->shard[s], back, h->st[s]);
            throw;
        }
    });
}

int rc_sharded_set_deep_select(rc_sharded *h, int kind) {
    return guard([&] {
        RC_REQUIRE(h, RC_ERR_INVALID, "null index");
        RC_REQUIRE(kind == RC_DEEP_SELECT_ROUNDS || kind == RC_DEEP_SELECT_RADIX, RC_ERR_INVALID,
                   "deep selection must be RC_DEEP_SELECT_ROUNDS or RC_DEEP_SELECT_RADIX");
        std::lock_guard<std::mutex> lk(h->mu);
        for (int s = 0; s < h->n; ++s) check_status(rc_index_set_deep_select(h->shard[s], kind));  // cannot fail: the kind is valid
        h->deep_select = kind;
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
            RC_REQUIRE(kind == RC_FILTER_NATIVE || kind == RC_FILTER_METRIC || kind == RC_FILTER_F32, RC_ERR_UNSUPPORTED,
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
            h->idx_h[s].get()[cnt[s]] = i;
            h->row_h[s].get()[cnt[s]] = g / h->n;
            ++cnt[s];
        }
        hipStream_t ls = (hipStream_t)stream;
        {
            // leader stream: source lists of every shard, then each remote shard's subset gathered
            // contiguous (cnt[s] rows, not the whole batch, cross xGMI)
            DeviceScope dl(h->dev[0]);
            for (int s = 0; s < h->n; ++s) {
                if (cnt[s] == 0) continue;
                RC_HIP(hipMemcpyAsync(h->idx_d[s].get(), h->idx_h[s].get(), cnt[s] * sizeof(int64_t), hipMemcpyHostToDevice, ls));
                if (h->remote[s]) {
                    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((cnt[s] + 3) / 4)), dim3(256), 0, ls, vecs,
                                       h->idx_d[s].get(), cnt[s], h->dim, h->gat_d[s].get());
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
            RC_HIP(hipMemcpyAsync(h->row_d[s].get(), h->row_h[s].get(), ms * sizeof(int64_t), hipMemcpyHostToDevice, h->st[s]));
            if (h->remote[s]) {
                RC_HIP(hipMemcpyPeerAsync(h->vec_d[s].get(), h->dev[s], h->gat_d[s].get(), h->dev[0], (size_t)ms * h->dim * sizeof(float),
                                          h->st[s]));
                index_upsert_gather(h->shard[s], h->vec_d[s].get(), nullptr, ms, h->row_d[s].get(), h->st[s]);
            } else {
                index_upsert_gather(h->shard[s], vecs, h->idx_d[s].get(), ms, h->row_d[s].get(), h->st[s]);
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
                h->mv_src_h[a].get()[soff[ab] + k] = gs / ns;
                h->mv_dst_h[b].get()[doff[ab] + k] = gd / ns;
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
                    RC_HIP(hipMemcpyAsync(h->mv_src_d[a].get(), h->mv_src_h[a].get(), s_tot[a] * sizeof(int64_t), hipMemcpyHostToDevice, sa));
                if (d_tot[a])
                    RC_HIP(hipMemcpyAsync(h->mv_dst_d[a].get(), h->mv_dst_h[a].get(), d_tot[a] * sizeof(int64_t), hipMemcpyHostToDevice, sa));
                const size_t aa = (size_t)a * ns + a;
                index_move_rows(h->shard[a], h->mv_src_d[a].get() + soff[aa], h->shard[a], h->mv_dst_d[a].get() + doff[aa], RowBlock{},
                                cnt[aa], sa);
                index_move_rows(h->shard[a], h->mv_src_d[a].get() + s_stg[a], nullptr, nullptr, h->mv_out[a].view(), s_tot[a] - s_stg[a], sa);
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
                        index_move_rows(h->shard[a], h->mv_src_d[a].get() + soff[ab], h->shard[b], h->mv_dst_d[b].get() + doff[ab],
                                        RowBlock{}, cnt[ab], sb);
                        continue;
                    }
                    const int64_t from = soff[ab] - s_stg[a], to = doff[ab] - d_stg[b];
                    RC_HIP(hipMemcpyPeerAsync((uint8_t *)h->mv_in[b].rows.get() + (size_t)to * rb, h->dev[b],
                                              (const uint8_t *)h->mv_out[a].rows.get() + (size_t)from * rb, h->dev[a],
                                              (size_t)cnt[ab] * rb, sb));
                    RC_HIP(hipMemcpyPeerAsync(h->mv_in[b].norms.get() + to, h->dev[b], h->mv_out[a].norms.get() + from, h->dev[a],
                                              (size_t)cnt[ab] * sizeof(float), sb));
                }
                index_move_rows(nullptr, nullptr, h->shard[b], h->mv_dst_d[b].get() + d_stg[b], h->mv_in[b].view(), d_tot[b] - d_stg[b], sb);
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
            h->idx_h[s].get()[cnt[s]] = i;  // destination row of out
            h->row_h[s].get()[cnt[s]] = g / h->n;
            ++cnt[s];
        }
        // every shard's fetch and D2H copy in flight at once, one wait at the end
        for (int s = 0; s < h->n; ++s) {
            if (cnt[s] == 0) continue;
            DeviceScope ds(h->dev[s]);
            const int64_t ms = cnt[s];
            RC_HIP(hipMemcpyAsync(h->row_d[s].get(), h->row_h[s].get(), ms * sizeof(int64_t), hipMemcpyHostToDevice, h->st[s]));
            check_status(stored ? rc_index_fetch_stored(h->shard[s], h->row_d[s].get(), ms, h->fo_d[s].get(), h->st[s])
                                : rc_index_fetch(h->shard[s], h->row_d[s].get(), ms, h->fo_d[s].get(), h->st[s]));
            RC_HIP(hipMemcpyAsync(h->fo_h[s].get(), h->fo_d[s].get(), (size_t)ms * h->dim * sizeof(float), hipMemcpyDeviceToHost,
                                  h->st[s]));
        }
        for (int s = 0; s < h->n; ++s) {
            if (cnt[s] == 0) continue;
            DeviceScope ds(h->dev[s]);
            RC_HIP(hipStreamSynchronize(h->st[s]));
            for (int64_t j = 0; j < cnt[s]; ++j)
                std::memcpy(out + h->idx_h[s].get()[j] * h->dim, h->fo_h[s].get() + j * h->dim, (size_t)h->dim * sizeof(float));
        }
}

// One result array of a fan-out, `bytes` per shard (nq x k entries): a single shard writes to `single`
// (the caller's own buffer), a shard on the leader's device to its slice of `gather` (leader,
// [n] slices), any other to loc[s] on its device, which is then peer-copied to that slice.
struct FanBuf {
    size_t bytes;
    void *single;
    void *gather;
    const DevBuf<void> *loc;
};

// The fan-out of a search over the shards (caller holds h->mu; `queries` on the leader, ls = the
// leader stream): the HOST mask over the global rows (optional) is staged per shard first, then
// every shard waits for the leader stream, takes the queries (a peer copy into qcopy[s] when it
// is remote), runs call(s, queries, its row count, its device mask, its nbuf outputs, its stream)
// and hands its results to the leader, whose stream waits for all of them.  Returns false when
// the one shard there is answered the caller directly, on ls (nothing is left to merge and the
// mask's words are free again), true with every buf's gather filled in stream order: the caller
// merges, then wait_mask()s if it gave a mask (the next call may overwrite the staged words).
template <typename Call>
bool fan_out(rc_sharded *h, const float *queries, int nq, int64_t n_rows, const uint32_t *mask, hipStream_t ls,
             const std::vector<DevBuf<float>> &qcopy, const FanBuf *buf, int nbuf, Call call) {
    const bool masked = mask != nullptr;
    if (masked) stage_mask(h, mask, n_rows, ls);
    void *out[2] = {nullptr, nullptr};
    if (h->n == 1) {
        for (int b = 0; b < nbuf; ++b) out[b] = buf[b].single;
        call(0, queries, n_rows, masked ? h->mk_d[0].get() : nullptr, out, ls);
        if (masked) {
            fence_mask_single(h, ls);
            wait_mask(h);
        }
        return false;
    }
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
            RC_HIP(hipMemcpyPeerAsync(qcopy[s].get(), h->dev[s], queries, h->dev[0], (size_t)nq * h->dim * sizeof(float), h->st[s]));
            q = qcopy[s].get();
        }
        for (int b = 0; b < nbuf; ++b) out[b] = local ? (uint8_t *)buf[b].gather + s * buf[b].bytes : buf[b].loc[s].get();
        call(s, q, shard_rows(h, s, n_rows), masked ? h->mk_d[s].get() : nullptr, out, h->st[s]);
        for (int b = 0; b < nbuf && !local; ++b)
            RC_HIP(hipMemcpyPeerAsync((uint8_t *)buf[b].gather + s * buf[b].bytes, h->dev[0], out[b], h->dev[s], buf[b].bytes, h->st[s]));
        RC_HIP(hipEventRecord(h->ev_done[s], h->st[s]));
    }
    DeviceScope dl(h->dev[0]);
    for (int s = 0; s < h->n; ++s) RC_HIP(hipStreamWaitEvent(ls, h->ev_done[s], 0));
    return true;
}

// rc_sharded_search's body (caller holds h->mu; device buffers on the leader, stream = leader stream)
// mask (optional): HOST bitmap over the global rows (fan_out).
// slot >= 0 (rc_sharded_search_pages): n_rows, the mask and the returned rows are positions of
// that slot; position i is on shard i % n as its position i / n, exactly as global rows are, so
// the split of the mask, the shards' row maps and the merge are the ones of the dense search.
void search_locked(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, float *scores, int64_t *out_rows,
                   int mode, void *stream, const uint32_t *mask = nullptr, int slot = -1) {
    if (h->n > 1) ensure_search(h, nq, k);
    const size_t slice = (size_t)nq * k;
    const FanBuf out[2] = {{slice * sizeof(float), scores, h->g_s.get(), h->s_loc.data()},
                           {slice * sizeof(int64_t), out_rows, h->g_r.get(), h->r_loc.data()}};
    const bool gathered = fan_out(h, queries, nq, n_rows, mask, (hipStream_t)stream, h->q, out, 2,
                                  [&](int s, const float *q, int64_t n_local, const uint32_t *m, void *const *o, hipStream_t st) {
        check_status(slot >= 0 ? rc_index_search_pages_ex(h->shard[s], q, nq, slot, n_local, k, m, (float *)o[0], (int64_t *)o[1], mode, st)
                               : rc_index_search_masked(h->shard[s], q, nq, n_local, k, m, (float *)o[0], (int64_t *)o[1], mode, st));
    });
    if (!gathered) return;
    DeviceScope dl(h->dev[0]);
    check_status(rc_topk_merge(h->g_s.get(), h->g_r.get(), h->n, nq, k, k, scores, out_rows, stream));
    if (mask != nullptr) wait_mask(h);
}

// rc_sharded_search_deep's body (caller holds h->mu; device buffers on the leader, stream = leader
// stream), as search_locked: the mask is a HOST bitmap over the global rows (slot >= 0: positions).
// Each shard selects its own k keys (global rows) with no traffic per round;
// the leader gathers the n lists and runs the same selection over those n x k keys.  A key's order
// does not depend on the shard that held the row, so the result is that of one index.  A single
// shard has no keys to gather: it writes scores / out_rows itself.
// sq (rc_sharded_search_hybrid, checked by the caller): the sparse queries, which every shard stages on
// its own device and adds to its scores before it selects; null: the deep search.
void search_deep_locked(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, float *scores, int64_t *out_rows,
                        void *stream, const uint32_t *mask, int slot, const SparseQueries *sq = nullptr) {
    hipStream_t ls = (hipStream_t)stream;
    if (h->n > 1) ensure_deep(h, nq, k);
    const FanBuf out{(size_t)nq * k * sizeof(uint64_t), nullptr, h->dg_keys.get(), h->dk_loc.data()};
    const bool gathered = fan_out(h, queries, nq, n_rows, mask, ls, h->dq, &out, 1,
                                  [&](int s, const float *q, int64_t n_local, const uint32_t *m, void *const *o, hipStream_t st) {
        index_search_deep(h->shard[s], q, nq, n_local, k, m, slot, (uint64_t *)o[0], scores, out_rows, st, sq);
    });
    if (!gathered) return;
    DeviceScope dl(h->dev[0]);
    const int qc = deep_chunk_queries(nq, (int64_t)h->n * k);
    h->dsel.ensure(qc, (int64_t)qc * k);
    for (int q0 = 0; q0 < nq; q0 += qc) {
        const int m = std::min(qc, nq - q0);
        DeepStream st;
        st.keys = h->dg_keys.get();  // list s of query q at [(s * nq + q) * k]
        st.n = (int64_t)h->n * k;
        st.klist = k;
        st.nq_total = nq;
        st.q0 = q0;
        deep_select(h->deep_select, st, h->dsel, m, k, h->dsel.keys.get(), ls);
        deep_emit(h->dsel.keys.get(), (int64_t)m * k, scores + (int64_t)q0 * k, out_rows + (int64_t)q0 * k, ls);
    }
    if (mask != nullptr) wait_mask(h);
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

// The table of a slot and the range of n_pos it covers, or an error (caller holds h->mu).
const std::vector<int32_t> &page_list(const rc_sharded *h, int slot, int64_t n_pos) {
    RC_REQUIRE(slot >= 0 && slot < (int)h->tables.size() && !h->tables[slot].empty(), RC_ERR_INVALID,
               "unknown slot (no page table was set for it)");
    const std::vector<int32_t> &L = h->tables[slot];
    RC_REQUIRE(n_pos >= 0 && n_pos <= (int64_t)L.size() * RC_PAGE_ROWS * h->n, RC_ERR_INVALID, "n_pos beyond the slot's pages");
    return L;
}

// What every sharded search entry point checks, and the lock its body runs under: the arguments
// (check_search_args: nothing reads *h before they passed), then under h->mu the range, global
// rows [0, n) or (slot >= 0) positions [0, n) of that slot.  A call without queries ends after this.
std::unique_lock<std::mutex> checked_lock(rc_sharded *h, int nq, int k, int k_max, bool buffers, int slot, int64_t n,
                                          int mode = RC_SEARCH_AUTO) {
    check_search_args(h, nq, k, k_max, buffers, mode);
    std::unique_lock<std::mutex> lk(h->mu);
    if (slot >= 0) (void)page_list(h, slot, n);
    else RC_REQUIRE(n >= 0 && n <= h->cap * h->n, RC_ERR_INVALID, "n_rows out of range");
    return lk;
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
        const auto lk = checked_lock(h, nq, k, RC_DEEP_TOPK_MAX, queries && scores && out_rows, -1, n_rows);
        if (nq == 0) return;
        const SparseQueries sq{sq_off, sq_idx, sq_val};
        check_hybrid(h, sq, nq);
        search_deep_locked(h, queries, nq, n_rows, k, scores, out_rows, stream, mask, -1, &sq);
    });
}

int rc_sharded_search_deep(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask, float *scores,
                           int64_t *out_rows, void *stream) {
    return guard([&] {
        const auto lk = checked_lock(h, nq, k, RC_DEEP_TOPK_MAX, queries && scores && out_rows, -1, n_rows);
        if (nq != 0) search_deep_locked(h, queries, nq, n_rows, k, scores, out_rows, stream, mask, -1);
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
        const auto lk = checked_lock(h, nq, k, RC_TOPK_MAX, queries && scores && out_rows, -1, n_rows);
        if (nq != 0) search_locked(h, queries, nq, n_rows, k, scores, out_rows, mode, stream, mask);
    });
}

int rc_sharded_query_host(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, int with_values,
                          float *scores, int64_t *out_rows, float *values) {
    return rc_sharded_query_host_masked(h, queries, nq, n_rows, k, with_values, nullptr, scores, out_rows, values);
}

int rc_sharded_query_host_masked(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, int with_values,
                                 const uint32_t *mask, float *scores, int64_t *out_rows, float *values) {
    return guard([&] {
        // (the lock is given back at once: query_host_checked takes it after its own early return)
        checked_lock(h, nq, k, RC_TOPK_MAX, queries && scores && out_rows && (!with_values || values), -1, n_rows);
        if (nq == 0) return;
        query_host_checked(h, queries, nq, n_rows, k, with_values, mask, scores, out_rows, values, -1);
    });
}

}  // extern "C"

namespace {

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
            // (refused, as for a shape outside its range, by a shard whose filter is RC_FILTER_I8_STREAM once the
            // rows reach that filter's AUTO bound: the multi-kernel path below then takes the streaming filter)
            float *hs = (float *)(h->qh.get() + L.sc);
            int64_t *hr = (int64_t *)(h->qh.get() + L.rw);
            float *hv = (float *)(h->qh.get() + L.val);
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
        std::memcpy(h->qh.get() + L.q, queries, (size_t)nq * h->dim * sizeof(float));
        RC_HIP(hipMemcpyAsync(h->qd.get() + L.q, h->qh.get() + L.q, (size_t)nq * h->dim * sizeof(float), hipMemcpyHostToDevice, h->qs));
        float *dsc = (float *)(h->qd.get() + L.sc);
        int64_t *drw = (int64_t *)(h->qd.get() + L.rw);
        search_locked(h, (const float *)(h->qd.get() + L.q), nq, n_rows, k, dsc, drw, slot >= 0 ? RC_SEARCH_SCAN : RC_SEARCH_AUTO, h->qs, mask,
                      slot);  // a slot scans, as before the paged batched search
        if (dev_values) {
            if (slot >= 0) index_fetch_pages(h->shard[0], slot, n_rows, drw, nk, (float *)(h->qd.get() + L.val), h->qs);
            else check_status(rc_index_fetch(h->shard[0], drw, nk, (float *)(h->qd.get() + L.val), h->qs));
        }
        RC_HIP(hipMemcpyAsync(h->qh.get() + L.sc, h->qd.get() + L.sc, (size_t)(L.total - L.sc), hipMemcpyDeviceToHost, h->qs));
        RC_HIP(hipStreamSynchronize(h->qs));
        std::memcpy(scores, h->qh.get() + L.sc, (size_t)nk * sizeof(float));
        std::memcpy(out_rows, h->qh.get() + L.rw, (size_t)nk * sizeof(int64_t));
        if (dev_values) {
            std::memcpy(values, h->qh.get() + L.val, (size_t)nk * h->dim * sizeof(float));
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
        const auto lk = checked_lock(h, nq, k, RC_TOPK_MAX, queries && scores && out_rows, paged_slot(slot), n_pos, mode);
        if (nq != 0) search_locked(h, queries, nq, n_pos, k, scores, out_rows, mode, stream, mask, slot);  // every shard takes the mode
    });
}

int rc_sharded_search_pages_deep(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k, const uint32_t *mask,
                                 float *scores, int64_t *out_rows, void *stream) {
    return guard([&] {
        const auto lk = checked_lock(h, nq, k, RC_DEEP_TOPK_MAX, queries && scores && out_rows, paged_slot(slot), n_pos);
        if (nq != 0) search_deep_locked(h, queries, nq, n_pos, k, scores, out_rows, stream, mask, slot);
    });
}

int rc_sharded_search_pages_hybrid(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k, const uint32_t *mask,
                                   const int32_t *sq_off, const uint32_t *sq_idx, const float *sq_val, float *scores,
                                   int64_t *out_rows, void *stream) {
    return guard([&] {
        const auto lk = checked_lock(h, nq, k, RC_DEEP_TOPK_MAX, queries && scores && out_rows, paged_slot(slot), n_pos);
        if (nq == 0) return;
        const SparseQueries sq{sq_off, sq_idx, sq_val};
        check_hybrid(h, sq, nq);
        search_deep_locked(h, queries, nq, n_pos, k, scores, out_rows, stream, mask, slot, &sq);
    });
}

int rc_sharded_query_host_pages(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k, int with_values,
                                const uint32_t *mask, float *scores, int64_t *out_rows, float *values) {
    return guard([&] {
        check_search_args(h, nq, k, RC_TOPK_MAX, queries && scores && out_rows && (!with_values || values));
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
