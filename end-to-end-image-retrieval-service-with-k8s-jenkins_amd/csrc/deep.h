// deep.h — deep top-k (rc_*_search_deep: exact results past RC_TOPK_MAX per query): what the host
// side (index.hip, sharded.hip) and the deep translation units share.  The score pass is in
// deep_scores.h (deep_scores_{f32,f16,bf16,f8}.hip), the bounded selection, its round chaining and
// the emit kernel in deep_select.hip.  DESIGN.md, "Deep top-k", has the argument for exactness.
#pragma once

#include <algorithm>

#include "index_common.h"

namespace rc {

// The score pass: the f32 score of every row (pages: position) r in [0, n_rows) of nq raw queries,
// to scores[q * n_rows + r] — scan_rows_q's loop (scan_rows_q_paged's with a page table) without
// the top-k and without a mask, each query normalised per wave as scan_rows does, so a score has
// the bits the scan's key carries.  grid.y = the query.
struct DeepScoreArgs {
    const void *rows;
    const float *norms;
    int64_t ld;
    int nch;
    int dim;
    int64_t n_rows;
    int64_t rows_per_block;
    int nblk;
    const float *queries;  // device f32 [nq][dim], raw
    int nq;
    int metric;
    const int32_t *pages;  // a slot's page table, or null (contiguous rows)
    float *scores;         // [nq][n_rows]
    hipStream_t stream;
};
template <typename T>
void launch_deep_scores(const DeepScoreArgs &a);  // deep_scores.h; instantiated in deep_scores_{f32,f16,bf16,f8}.hip

// The key stream a selection runs over, n entries per query.  Either
//   scores: f32 [nq][n], entry r keyed make_key(scores[q][r], row_base + r * row_stride), eligible
//           iff bit r of mask is set (mask may be null: every entry), or
//   keys:   nlist lists of klist ready keys per query, list l of query q at
//           keys[(l * nq_total + q0 + q) * klist], entry i = key i % klist of list i / klist
//           (KEY_EMPTY entries are skipped; no mask).
struct DeepStream {
    const float *scores = nullptr;
    const uint64_t *keys = nullptr;
    int64_t n = 0;
    int64_t row_base = 0, row_stride = 1;
    const uint32_t *mask = nullptr;
    int klist = 1, nq_total = 1, q0 = 0;
};

// The selection's workspace for up to nq queries in flight: the blocks' partial lists, the
// rounds' lower bounds and (ensure's with_keys) k keys per query.  Grows, never shrinks.
struct DeepSel {
    int nq_cap = 0;
    int64_t keys_cap = 0;
    uint64_t *partial = nullptr;  // [DEEP_SELECT_BLOCKS][nq_cap][RC_TOPK_MAX]
    uint64_t *lower = nullptr;    // [nq_cap]
    uint64_t *keys = nullptr;     // [keys_cap]
    void ensure(int nq, int64_t nkeys);
    void release();
};
constexpr int DEEP_SELECT_BLOCKS = 256;  // partial lists per query, at most

// queries in flight for score arrays of n entries each (the documented workspace bound)
inline int deep_chunk_queries(int nq, int64_t n) {
    const int64_t fit = std::max<int64_t>(1, RC_DEEP_WS_BYTES / std::max<int64_t>(4, 4 * n));
    return (int)std::min<int64_t>(std::min<int64_t>(nq, RC_DEEP_CHUNK_QUERIES), fit);
}

// Enqueue every round of the selection of the k smallest keys of nq streams (nq <= ws.nq_cap) on
// `s`: out_keys[q * k + j] = the j-th key, KEY_EMPTY past the eligible entries.  No host wait.
void deep_select_rounds(const DeepStream &st, DeepSel &ws, int nq, int k, uint64_t *out_keys, hipStream_t s);
// keys -> (score, row) by RC_EMIT_KEY with base 0 and stride 1 (the keys carry global rows)
void deep_emit(const uint64_t *keys, int64_t n, float *scores, int64_t *rows, hipStream_t s);

}  // namespace rc
