// sparse.h — sparse-dense hybrid scores (rc_*_search_hybrid; DESIGN.md, "Sparse-dense hybrid"):
// what the host side (index.hip, sharded.hip) and sparse_add.hip share.  A shard's store holds
// `width` (index, value) slots per local row, slot-major; the add kernel runs between the deep
// top-k's score pass and its selection (deep.h) and adds each row's sparse term to its f32 score.
#pragma once

#include <functional>

#include "rc_common.h"

namespace rc {

constexpr uint32_t SPARSE_PAD = 0xFFFFFFFFu;  // the index of an unused slot; no record or query may carry it

// The store of one rc_index: slot j of local row r at idx[j * capacity + r] / val[j * capacity + r],
// a row's slots ascending by index and padded with SPARSE_PAD (value 0).  width == 0: not enabled.
struct SparseStore {
    uint32_t *idx = nullptr;
    float *val = nullptr;
    int width = 0;
};

// Sparse queries as HOST CSR: query q holds entries [off[q], off[q + 1]) of idx / val, its indices
// strictly ascending, none SPARSE_PAD, at most RC_SPARSE_MAX_NNZ of them.
struct SparseQueries {
    const int32_t *off;
    const uint32_t *idx;
    const float *val;
};
// Throws RC_ERR_INVALID unless sq is what the comment above says, for nq queries.
void sparse_check_queries(const SparseQueries &sq, int nq);

// A shard's device copy of the sparse queries of one call and the staging of a store write: pinned
// host blocks, their device twins and the event after which the pinned words are free again.
// Grows, never shrinks.
struct SparseWs {
    int64_t q_cap = 0, off_cap = 0;  // entries / offsets of the query copy
    int32_t *off_h = nullptr, *off_d = nullptr;
    uint32_t *idx_h = nullptr, *idx_d = nullptr;
    float *val_h = nullptr, *val_d = nullptr;
    int64_t w_rows = 0, w_slots = 0;  // rows / slots (rows x width) of one write round
    int64_t *wrow_h = nullptr, *wrow_d = nullptr;
    uint32_t *widx_h = nullptr, *widx_d = nullptr;
    float *wval_h = nullptr, *wval_d = nullptr;
    hipEvent_t ev = nullptr;
    bool pending = false;  // ev was recorded and not waited for yet
    void wait();           // until the last staged copy left the pinned blocks
    void stage_queries(const SparseQueries &sq, int nq, hipStream_t s);
    void ensure_write(int64_t rows, int width);
    void release();
};

// scores[q * n + r] = fadd(scores[q * n + r], t(q0 + q, row of r)) for q in [0, nq), r in [0, n):
// r is a local row, or with a page table a position whose row is pages[r / 256] * 256 + r % 256.
// A row without stored entries and every row under a query without entries keep their bits.
struct SparseAddArgs {
    const uint32_t *s_idx;
    const float *s_val;
    int width;
    int64_t capacity;
    const int32_t *q_off;  // device CSR of the call's queries
    const uint32_t *q_idx;
    const float *q_val;
    int q0, nq;
    int64_t n;
    const int32_t *pages;  // or null
    float *scores;
    hipStream_t stream;
};
void launch_sparse_add(const SparseAddArgs &a);
// slots [0, width) of row rows[i] = in_idx / in_val[i * width ..]; a row outside [0, capacity) is skipped
void launch_sparse_scatter(const SparseStore &st, int64_t capacity, const int64_t *rows, const uint32_t *in_idx, const float *in_val,
                           int64_t n, hipStream_t s);
// a store of new_cap rows per slot from one of old_cap: the old rows copied, the new ones padded
void launch_sparse_regrow(const SparseStore &from, int64_t old_cap, uint32_t *idx, float *val, int64_t new_cap, hipStream_t s);

// The step the hybrid searches hand the deep search (deep_search_locked): after the score pass of
// the queries [q0, q0 + m) of the call, over their score array [m][n].
using DeepAfterScores = std::function<void(int q0, int m, float *scores, hipStream_t s)>;

}  // namespace rc
