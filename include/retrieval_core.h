/*
 * retrieval_core.h — C ABI of the MI355X-native retrieval core.
 *
 * One hipcc-built shared library (libretrieval_core.so, gfx950) behind the
 * reference's own API for the hot path "embed a batch of images → exact cosine
 * top-k over an in-HBM index".  The reference has no FFI of its own: its hot
 * path is remote Python (transformers in the embedding pod, Pinecone SaaS for
 * the index).  Each entry point below names the reference call it replaces;
 * INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every function returns int status (RC_OK = 0); on error the message is
 *     in the thread-local rc_last_error(); no C++ exception crosses the ABI;
 *   - device buffers are caller-owned (e.g. torch tensors' data_ptr) unless a
 *     function says otherwise; `stream` is a hipStream_t (NULL = default);
 *   - hot calls (rc_index_search, rc_index_upsert, rc_embed) allocate nothing
 *     once the workspace is reserved (rc_index_reserve / rc_model_create);
 *   - each handle is bound to the device it was created on and guarded by a
 *     mutex, so a multi-threaded caller may share it.
 */
#ifndef RETRIEVAL_CORE_H
#define RETRIEVAL_CORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ABI_VERSION 1

/* status codes */
#define RC_OK 0
#define RC_ERR_INVALID 1     /* bad argument (maps to ValueError)            */
#define RC_ERR_HIP 2         /* HIP runtime failure                          */
#define RC_ERR_OOM 3         /* device allocation failed                     */
#define RC_ERR_UNSUPPORTED 4 /* valid request outside what the build handles */
#define RC_ERR_STATE 5       /* handle not ready (e.g. weights missing)      */

/* storage dtypes of index rows */
#define RC_F32 0
#define RC_F16 1
#define RC_BF16 2
/* float8: each element is the OCP e4m3fn byte (round to nearest even) of x̂_c · 2⁸, the stored
 * value is decode(byte) · 2⁻⁸ (3 mantissa bits; |x̂_c| <= 1, so nothing saturates, and elements
 * down to 2⁻¹⁴ stay normal).  One byte per element, ld = round_up(dim, 256).  It scans exactly
 * by default: RC_SEARCH_MFMA is RC_ERR_UNSUPPORTED and RC_SEARCH_AUTO scans until its own filter
 * is switched on, rc_index_set_filter(RC_FILTER_F8) (cosine, ld 256 / 512 / 768), which gives it
 * the batched search with unchanged results.  RC_FILTER_I8 is RC_ERR_UNSUPPORTED on it. */
#define RC_F8 3

/* Pillow resampling filters (PIL.Image.Resampling values) */
#define RC_RESAMPLE_BILINEAR 2
#define RC_RESAMPLE_BICUBIC 3

#define RC_TOPK_MAX 256 /* largest k a single search call accepts */

typedef struct rc_index rc_index;
typedef struct rc_sharded rc_sharded;
typedef struct rc_model rc_model;

const char *rc_last_error(void);
int rc_abi_version(void);
/* Device and pinned-host allocations the library has made so far (all handles).
 * Diagnostic: the tests check that steady-state hot calls (search, fetch,
 * upsert, embed once their workspaces exist) leave it unchanged. */
int64_t rc_alloc_count(void);

/* ------------------------------------------------------------------------
 * In-HBM exact cosine index.  Replaces the Pinecone index:
 *   get_index(name)            ingesting/utils.py:23-38, retriever/utils.py:23-38
 *   index.upsert([(id,v,md)])  ingesting/main.py:156-158
 *   index.query(v, top_k)      retriever/utils.py:62-64
 *   index.fetch(ids)           retriever/main.py:142
 * Rows are stored L2-normalised in `dtype`, row-major with leading dimension
 * ld = round_up(dim, 128) (round_up(dim, 256) for RC_F8; zero padded).  String ids and metadata stay on the
 * host; the device only knows row numbers.  A search returns
 * row_base + local_row * row_stride (row_stride = 1 unless rc_index_set_row_map
 * says otherwise): the global row of a shard in a multi-GPU index.
 * ---------------------------------------------------------------------- */

/* replaces pc.create_index(metric="cosine", dimension=dim) — ingesting/utils.py:29-36 */
int rc_index_create(int device, int dim, int dtype, int64_t capacity, int64_t row_base, rc_index **out);
int rc_index_destroy(rc_index *h);
int rc_index_info(const rc_index *h, int *dim, int *dtype, int64_t *capacity, int64_t *ld);
/* device pointer to row 0 of the stored (normalised, cast) rows */
int rc_index_data(const rc_index *h, void **rows_dev, float **norms_dev);

/* Shard row map: local row l is reported as row_base + l * row_stride (a
 * round-robin shard s of n uses row_base = s, row_stride = n). */
int rc_index_set_row_map(rc_index *h, int64_t row_base, int64_t row_stride);

/* Grow the row capacity in place (rows and norms are copied to a larger
 * allocation; new slots are zero).  Pinecone indexes have no fixed capacity
 * (ingesting/utils.py:29-36 creates one without a size); the host layer grows
 * on demand.  The caller orders earlier work on other streams; the call
 * synchronises the device before releasing the old buffers. */
int rc_index_grow(rc_index *h, int64_t new_capacity, void *stream);

/* Size the search workspace for up to max_nq queries and k <= max_k.  Called
 * once before the hot loop; search grows it on demand otherwise. */
int rc_index_reserve(rc_index *h, int max_nq, int max_k);

/* replaces index.upsert — ingesting/main.py:156-158.
 * vecs: device f32 [n, dim]; rows: device i64 [n] local row slots (host-assigned:
 * an existing id keeps its row, so upsert overwrites).  Each row is L2-normalised
 * in f32, cast to the storage dtype and scattered; its norm is kept so fetch can
 * return the original values.  An all-zero vector is rejected by the host layer.
 * Rows must be distinct within one call (one wave per vector writes its row: a
 * repeated row would interleave two vectors); Index.upsert keeps the last
 * occurrence of a repeated id before calling. */
int rc_index_upsert(rc_index *h, const float *vecs, int64_t n, const int64_t *rows, void *stream);

/* The device half of index.delete(ids) (Pinecone's call; the reference never deletes):
 * the host layer keeps the live rows dense by swap-remove (Index.delete fills each
 * hole below the new length with a surviving row of the tail) and this moves the rows.
 * src_rows, dst_rows: device i64 [n] local rows; stored row dst_rows[i] becomes a
 * bit-for-bit copy of stored row src_rows[i] (ld elements and the norm), and the
 * int8 filter copy of the written rows is refreshed as upsert refreshes it.
 * Precondition: the two lists are disjoint (no row is both read and written) and
 * dst_rows holds no row twice (one wave per row: two writers of one row would
 * interleave).  A row outside [0, capacity) in either list skips that pair on the
 * device; the hosts validate first. */
int rc_index_move_rows(rc_index *h, const int64_t *src_rows, const int64_t *dst_rows, int64_t n, void *stream);

/* replaces index.fetch(ids)["vectors"][id]["values"] — retriever/main.py:142.
 * rows: device i64 [n]; out: device f32 [n, dim] = stored row × stored norm. */
int rc_index_fetch(rc_index *h, const int64_t *rows, int64_t n, float *out, void *stream);
/* The stored (normalised, dtype-rounded) rows as f32, without the norm —
 * what the search actually scores against (parity tests run the oracle on these). */
int rc_index_fetch_stored(rc_index *h, const int64_t *rows, int64_t n, float *out, void *stream);

/* Snapshot / restore (Pinecone keeps an index durable server-side; the in-HBM
 * index is saved by the host layer — Index.save / Index.load — through these).
 * Raw copy of the stored rows [row0, row0+n) exactly as searched (storage dtype,
 * ld-padded, normalised) and their norms.  Buffers may be device or host memory
 * (hipMemcpyDefault); the copy is ordered on `stream`. */
int rc_index_export(rc_index *h, int64_t row0, int64_t n, void *rows_out, float *norms_out, void *stream);
int rc_index_import(rc_index *h, int64_t row0, int64_t n, const void *rows_in, const float *norms_in, void *stream);

/* replaces index.query(vector, top_k) — retriever/utils.py:62-64.
 * queries: device f32 [nq, dim] (normalised inside); rows [0, n_rows) are searched.
 * scores: device f32 [nq, k] cosine, descending; out_rows: device i64 [nq, k]
 * (global rows, see the row map).  Ties: score desc, then row asc.  Slots beyond
 * n_rows get score -inf and row -1 (n_rows = 0, an empty shard, is valid in
 * every mode).  1 <= k <= RC_TOPK_MAX; a larger top_k is RC_ERR_INVALID. */
int rc_index_search(rc_index *h, const float *queries, int nq, int64_t n_rows, int k,
                    float *scores, int64_t *out_rows, void *stream);

/* Search algorithm selection for rc_index_search_ex (same results either way):
 *   RC_SEARCH_SCAN — HBM-bound streaming scan, 1-4 queries per pass over the rows;
 *   RC_SEARCH_MFMA — batched: query-block x row-tile MFMA GEMM (f16/bf16 index only)
 *                    whose epilogue keeps candidates within a proven error bound
 *                    of the running kth score, exact f32 rescoring of candidates;
 *                    a query whose candidates overflow is re-run through the
 *                    exact scan ON THE DEVICE (no host synchronisation);
 *   RC_SEARCH_AUTO — MFMA for >= 8 queries on an f16/bf16 index of >= 64k rows.
 * This is the batched form of index.query (retriever/utils.py:62-64) that
 * BASELINE config 4 (1024 queries, top-100) exercises. */
#define RC_SEARCH_AUTO 0
#define RC_SEARCH_SCAN 1
#define RC_SEARCH_MFMA 2
#define RC_SEARCH_MFMA_MASKED 3 /* rc_index_search_masked: RC_SEARCH_MFMA with the mask inside the filter GEMM */
int rc_index_search_ex(rc_index *h, const float *queries, int nq, int64_t n_rows, int k,
                       float *scores, int64_t *out_rows, int mode, void *stream);

/* replaces index.query(vector, top_k, filter={...}) — the row-eligibility form of
 * rc_index_search_ex (the reference never passes Pinecone's `filter`; users of a
 * Pinecone-shaped index do).  The host evaluates the metadata predicate; the device
 * gets a bitmap and restricts the exact search to the eligible rows INSIDE the scan.
 * mask: device u32 [ceil(n_rows/32)], bit (r & 31) of word r >> 5 = local row r is
 * eligible; bits at or past n_rows are ignored.  NULL = rc_index_search_ex.
 * Same contract otherwise: an eligible row's score is bit-identical to the unmasked
 * search's, ties order by row, slots past the eligible rows get -inf / -1 (a mask
 * with no eligible row is valid).  Modes: RC_SEARCH_SCAN skips the row loads of
 * every 8-row group (16-row on an RC_F8 index) without an eligible row; RC_SEARCH_MFMA keeps the filter GEMM
 * as it is and drops ineligible candidates when rescoring (overflowed queries fall
 * back to the masked scan on the device); RC_SEARCH_MFMA_MASKED also applies the mask in
 * the filter GEMM's epilogue, so the candidate lists hold eligible rows only and a
 * selective mask no longer overflows them (a clustered one still can, and falls back);
 * it is refused exactly where RC_SEARCH_MFMA is and equals it without a mask;
 * RC_SEARCH_AUTO with a mask scans. */
int rc_index_search_masked(rc_index *h, const float *queries, int nq, int64_t n_rows, int k,
                           const uint32_t *mask, float *scores, int64_t *out_rows, int mode, void *stream);

/* Filter copy for the batched search (no reference counterpart: Pinecone's query
 * internals; results are unchanged, only the speed of RC_SEARCH_MFMA):
 *   RC_FILTER_NATIVE — the filter GEMM reads the stored rows (f16/bf16 MFMA);
 *   RC_FILTER_I8     — the index also keeps an int8 copy of every row (per-row
 *                      scale and residual norm, ld + 8 bytes per row, maintained
 *                      by upsert / fill / import / grow); the filter GEMM runs on
 *                      int8 MFMA at twice the f16 rate with a per-(query, row) error
 *                      bound, and candidates are rescored exactly on the stored rows.
 *                      Row widths (dim rounded up to 128) 256, 512 or 768; makes
 *                      RC_SEARCH_MFMA available on f32 indexes too.
 *                      Enabling quantises every row (synchronous on `stream`).
 *   RC_FILTER_F8     — an RC_F8 index only: the filter GEMM reads the stored e4m3
 *                      rows with the block-scaled fp8 MFMA (twice the f16 rate, half
 *                      the row bytes), the query held as two e4m3 terms; candidates
 *                      are rescored exactly on the stored rows, so RC_SEARCH_MFMA
 *                      returns the scan's rows and score bits.  It allocates nothing;
 *                      RC_FILTER_NATIVE switches it off.  With it RC_SEARCH_MFMA is
 *                      available and RC_SEARCH_AUTO takes the batched path under its
 *                      usual conditions.  RC_ERR_UNSUPPORTED on an index that is not
 *                      RC_F8, not cosine, or of a row width (dim rounded up to 256)
 *                      other than 256, 512 or 768.
 *   RC_FILTER_METRIC — an RC_F16 / RC_BF16 index only (RC_ERR_UNSUPPORTED on any other):
 *                      the batched search under every metric.  Under RC_METRIC_COSINE it
 *                      is RC_FILTER_NATIVE: the same kernels, the same bits.  Under
 *                      RC_METRIC_DOT / RC_METRIC_EUCLIDEAN the same filter GEMM over the
 *                      stored rows bounds each row's METRIC score from above (from the
 *                      GEMM's value, its error bound and the row's norm) and keeps the
 *                      rows whose bound reaches the query's running k-th best metric
 *                      score; candidates are rescored exactly by the metric's rule, so
 *                      RC_SEARCH_MFMA returns the scan's rows and score bits, and
 *                      RC_SEARCH_AUTO takes the batched path under its usual
 *                      conditions.  It allocates nothing (switching to it from
 *                      RC_FILTER_I8 frees the int8 copy); all three metrics may be set
 *                      on it, in any order. */
#define RC_FILTER_NATIVE 0
#define RC_FILTER_I8 1
#define RC_FILTER_F8 2
#define RC_FILTER_METRIC 3
int rc_index_set_filter(rc_index *h, int kind, void *stream);
int rc_index_get_filter(const rc_index *h, int *kind);
/* What the RC_FILTER_F8 filter computes (a diagnostic: no reference counterpart).  Runs the
 * filter's query preparation and its kernel's own K loop over the local rows
 * [row0, row0 + n) (row0 a multiple of 128) and writes the filter scores s' — the two-term
 * e4m3 query against the stored rows, before any threshold — to out_scores (device f32
 * [nq][n]) and each query's bound on |s' − exact score| to out_eps (device f32 [nq]).
 * queries: device f32 [nq][dim].  RC_ERR_UNSUPPORTED unless the filter kind is RC_FILTER_F8. */
int rc_index_filter_scores(rc_index *h, const float *queries, int nq, int64_t row0, int64_t n, float *out_scores,
                           float *out_eps, void *stream);

/* replaces the metric= argument of pc.create_index — ingesting/utils.py:29-36 (the
 * reference asks for "cosine"; Pinecone also offers "dotproduct" and "euclidean").
 * The metric is a scoring rule over unchanged storage: setting it touches no data,
 * applies to later searches and is legal on a populated index.  Every stored row r is
 * an L2-normalised direction x̂_r in the storage dtype plus its f32 norm n_r, and
 * v_r = x̂_r · n_r is the vector rc_index_fetch returns; q is the raw query.
 *   RC_METRIC_COSINE    — the default, as documented at rc_index_search;
 *   RC_METRIC_DOT       — score = q · v_r, higher is better, best first;
 *   RC_METRIC_EUCLIDEAN — the SQUARED distance ‖q − v_r‖², as Pinecone reports it,
 *                         lower is better.  Every search keeps its contract of
 *                         returning scores descending: the library returns
 *                         s = −‖q − v_r‖², most similar first, and the host layer
 *                         reports max(0, −s), so its scores ascend.
 * Ties order by ascending row under every metric.  The top-k is chosen by the metric's
 * score inside the exact scan (never a re-ranked cosine top-k): with c the row's exact
 * cosine, ss the f32 sum of squares of q and qn = sqrtf(ss), the score is
 * s = fmaf(n_r, fmaf(alpha, c, −(beta · n_r)), −gamma) with (alpha, beta, gamma) =
 * (qn, 0, 0) for RC_METRIC_DOT and (2 qn, 1, ss) for RC_METRIC_EUCLIDEAN.  It is a
 * function of the row and the query alone: every search path and a sharded index give
 * the same bits.  All-zero vectors and queries stay rejected by the host layer.
 * The batched MFMA path serves a non-cosine metric only through RC_FILTER_METRIC (an
 * f16 / bf16 index), whose filter bounds the metric's own score per row.  With any other
 * filter kind its candidate threshold is a bound in cosine space: on a non-cosine index
 * with RC_FILTER_NATIVE RC_SEARCH_AUTO scans and RC_SEARCH_MFMA is RC_ERR_UNSUPPORTED;
 * rc_index_set_filter(RC_FILTER_I8 / RC_FILTER_F8) on a non-cosine index is
 * RC_ERR_UNSUPPORTED (those two filters are cosine-only), and so is a non-cosine metric
 * on an index whose filter is RC_FILTER_I8 or RC_FILTER_F8.  An unknown metric is
 * RC_ERR_INVALID. */
#define RC_METRIC_COSINE 0
#define RC_METRIC_DOT 1
#define RC_METRIC_EUCLIDEAN 2
int rc_index_set_metric(rc_index *h, int metric);
int rc_index_get_metric(const rc_index *h, int *metric);

/* Synthetic rows for benchmarks (no reference counterpart): rows
 * [row0, row0+n) get uniform[-1,1) values from a counter-based hash of
 * (seed, row, col), normalised and cast like an upsert. */
int rc_index_fill_random(rc_index *h, uint64_t seed, int64_t row0, int64_t n, void *stream);

/* Merge nlists top-k lists per query into one (cross-shard merge after the
 * all-gather; no reference counterpart — Pinecone merges server-side).
 * scores/rows: device [nlists, nq, k_in] of (score, global row); rows < 0 are
 * empty slots; global rows must be < 2^32 - 1 (every rc_index row map is
 * checked against that bound at create / set_row_map / grow).  Result ordered score desc, then
 * row asc — whatever the routing of rows to lists.  out: device [nq, k]. */
int rc_topk_merge(const float *scores, const int64_t *rows, int nlists, int nq, int k_in, int k,
                  float *out_scores, int64_t *out_rows, void *stream);

/* ------------------------------------------------------------------------
 * One index over several shards in one process (SURVEY §8(b):
 * rc_index_create(dim, dtype, capacity_per_gpu, n_gpus)).  Shard s is an
 * rc_index on devices[s] (devices may repeat: several shards on one GPU);
 * global row g lives on shard g % n_shards as local row g / n_shards
 * (round-robin, so every shard fills from the first upsert).  Queries and
 * results live on devices[0] (the leader); shards search concurrently on their
 * own streams and their lists are merged on the leader (rc_topk_merge).
 * Total capacity < 2^32 rows.
 * ---------------------------------------------------------------------- */
int rc_sharded_create(int n_shards, const int *devices, int dim, int dtype, int64_t capacity_per_shard,
                      rc_sharded **out);
int rc_sharded_destroy(rc_sharded *h);
/* Test hook: drive every shard but the leader through the cross-device path (subset
 * gather on the leader, peer copies of queries / subsets / result lists, leader merge)
 * even where shards share the leader's GPU — the code an 8-GPU node runs, on one GPU. */
int rc_sharded_force_remote(rc_sharded *h);
int rc_sharded_info(const rc_sharded *h, int *n_shards, int64_t *capacity_per_shard, int64_t *ld);
/* Borrowed handle of shard s (persistence, parity tests); owned by h. */
int rc_sharded_shard(rc_sharded *h, int s, rc_index **out);
int rc_sharded_grow(rc_sharded *h, int64_t new_capacity_per_shard);
/* replaces index.upsert — ingesting/main.py:156-158.  vecs: leader-device f32
 * [n, dim]; rows: HOST i64 [n] global rows.  Synchronous (ordered after work
 * already queued on `stream`). */
int rc_sharded_upsert(rc_sharded *h, const float *vecs, int64_t n, const int64_t *rows, void *stream);
/* rc_index_move_rows over the shards (index.delete's compaction).  src_rows, dst_rows:
 * HOST i64 [n] global rows; stored row dst_rows[i] becomes a copy of stored row
 * src_rows[i].  Before any device call the lists are validated: every row within
 * capacity, no row twice in src_rows, none twice in dst_rows, none in both — else
 * RC_ERR_INVALID and nothing has moved.  Pairs on one shard move inside it; pairs
 * between two shards of one GPU move in one launch; pairs between GPUs are packed into
 * a staging block on the source GPU, copied straight to the destination GPU and unpacked
 * there.  Staging (stored bytes, ld * sizeof(dtype) + 4 per row) grows on demand and is
 * bounded: long lists run in rounds of 16384 rows.  Synchronous. */
int rc_sharded_move_rows(rc_sharded *h, const int64_t *src_rows, const int64_t *dst_rows, int64_t n);
/* replaces index.fetch — retriever/main.py:142.  rows: HOST i64 [n] global rows;
 * out: HOST f32 [n, dim] (stored = 0: the upserted values; 1: the normalised
 * stored rows the search scores).  Synchronous. */
int rc_sharded_fetch(rc_sharded *h, const int64_t *rows, int64_t n, float *out, int stored);
/* replaces index.query — retriever/utils.py:62-64.  queries: leader-device f32
 * [nq, dim]; n_rows: global rows [0, n_rows) are searched; scores / out_rows:
 * leader-device [nq, k], identical to one rc_index holding the same rows. */
int rc_sharded_search(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, float *scores,
                      int64_t *out_rows, int mode, void *stream);
/* replaces index.query(vector, top_k, include_values=True) on the request path —
 * retriever/utils.py:62-64 (the call retriever/main.py:127-130 times).  Host in,
 * host out: queries HOST f32 [nq, dim]; scores HOST f32 [nq, k], out_rows HOST i64
 * [nq, k] (global rows, -1 past the index), values HOST f32 [nq, k, dim] (the
 * upserted values of each match, NaN for -1 slots; only when with_values).  One
 * H2D copy, the search, the matched rows' gather and ONE D2H copy on the index's
 * own leader stream, then one synchronisation; no allocation once the staging
 * has grown to the call's size.  Results equal rc_sharded_search +
 * rc_sharded_fetch. */
int rc_sharded_query_host(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, int with_values,
                          float *scores, int64_t *out_rows, float *values);
/* The masked forms of rc_sharded_search / rc_sharded_query_host (index.query with
 * filter=...).  mask: HOST u32 [ceil(n_rows/32)] over GLOBAL rows (as
 * rc_sharded_upsert takes host rows), bit (g & 31) of word g >> 5 = global row g is
 * eligible; NULL = the unmasked call.  The library de-interleaves it into one local
 * bitmap per shard (global row g = local row g / n of shard g % n) in pinned staging
 * and copies each to its shard's device on that shard's stream; no allocation once
 * the staging has grown to the call's size.  The call returns once the staged
 * bitmaps were copied (the host words may be reused at once); the search itself is
 * ordered on `stream` as rc_sharded_search's is.  The masked query_host always takes
 * the multi-kernel path (no masked form of the one-launch single-query path). */
int rc_sharded_search_masked(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k,
                             const uint32_t *mask, float *scores, int64_t *out_rows, int mode, void *stream);
int rc_sharded_query_host_masked(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k,
                                 int with_values, const uint32_t *mask, float *scores, int64_t *out_rows,
                                 float *values);
/* rc_index_set_filter on every shard; all or nothing (a failure restores
 * RC_FILTER_NATIVE on every shard, or RC_FILTER_METRIC if that was the kind before). */
int rc_sharded_set_filter(rc_sharded *h, int kind);
/* rc_index_set_metric on every shard; the metric is validated against every shard
 * before any is set (an unknown metric, or a shard whose filter is neither RC_FILTER_NATIVE nor RC_FILTER_METRIC under a non-cosine metric, changes none). */
int rc_sharded_set_metric(rc_sharded *h, int metric);

/* ------------------------------------------------------------------------
 * Page tables: several independent vector sets (namespaces) in one index's rows.
 *
 * A slot names one set.  Its vectors are dense in POSITION space [0, n_pos); the
 * rows are handed out in pages of RC_PAGE_ROWS local rows per shard, and the slot's
 * page table lists its pages in position order.  On one rc_index, position p lives
 * at local row pages[p / RC_PAGE_ROWS] * RC_PAGE_ROWS + p % RC_PAGE_ROWS.  On an
 * rc_sharded handle of S shards one page number means local rows
 * [RC_PAGE_ROWS p, RC_PAGE_ROWS (p + 1)) on EVERY shard, i.e. global rows
 * [RC_PAGE_ROWS S p, RC_PAGE_ROWS S (p + 1)): position i lives at global row
 * pages[i / (RC_PAGE_ROWS S)] * RC_PAGE_ROWS S + i % (RC_PAGE_ROWS S), on shard
 * i % S, as that shard's position i / S.  Rows are written, read and moved by global
 * row through the calls above; only the searches below go through the table.
 *
 * A paged search scores positions [0, n_pos) and returns POSITIONS: scores, positions
 * and tie order are bit-identical to a dense index of S shards holding the same
 * vectors in position order, searched with RC_SEARCH_SCAN (the scan kernels' paged
 * form; the same merges).  Rows of the last page at or past n_pos are never scored.
 * mask: a bitmap over positions (as rc_index_search_masked / rc_sharded_search_masked
 * over rows), or NULL.
 *
 * rc_*_search_pages_ex takes a search mode, one of RC_SEARCH_*, as rc_index_search_masked
 * does; rc_*_search_pages is RC_SEARCH_SCAN.  RC_SEARCH_MFMA / RC_SEARCH_MFMA_MASKED run
 * the batched MFMA search over the slot's pages (the page-table forms of the native
 * f16 / bf16 filter, rescore and fallback kernels; cosine, or dotproduct / euclidean with
 * RC_FILTER_METRIC): the same bits as RC_SEARCH_SCAN, ties included.  They return
 * RC_ERR_UNSUPPORTED where rc_index_search_ex refuses them and on an index whose filter
 * is RC_FILTER_I8 or RC_FILTER_F8, which have no paged form.  RC_SEARCH_MFMA_MASKED
 * without a mask is RC_SEARCH_MFMA; with one it is refused (RC_ERR_UNSUPPORTED) under a
 * non-cosine metric at row width 512, the one form that is not built.  RC_SEARCH_AUTO scans with a mask, and without one
 * takes the batched search where it is available and measured ahead of the paged scan:
 * from 64 queries over 65536 positions per shard, or 16 queries over 262144 (DESIGN.md,
 * "Namespaces").  An unknown mode is RC_ERR_INVALID.  Queries
 * whose candidates overflow count in rc_index_gemm_timing_read's fallbacks.
 *
 * rc_*_pages_set installs or replaces a slot's table (n_pages = 0 frees it): a
 * device-resident int32 array per shard, one allocation per slot and shard, doubled
 * when it grows.  It waits for the device, so call it when a set gains or loses a
 * page, not per query.  Every argument is checked before any device call: a slot
 * outside [0, RC_PAGE_SLOTS_MAX) or without a table, n_pos beyond the table's
 * pages, a page at or past capacity / RC_PAGE_ROWS, k outside [1, RC_TOPK_MAX] and
 * NULL buffers return RC_ERR_INVALID. */
#define RC_PAGE_ROWS 256
#define RC_PAGE_SLOTS_MAX 1048576
int rc_index_pages_set(rc_index *h, int slot, const int32_t *pages_host, int n_pages, void *stream);
int rc_index_search_pages(rc_index *h, const float *queries, int nq, int slot, int64_t n_pos, int k,
                          const uint32_t *mask, float *scores, int64_t *out_rows, void *stream);
int rc_index_search_pages_ex(rc_index *h, const float *queries, int nq, int slot, int64_t n_pos, int k,
                             const uint32_t *mask, float *scores, int64_t *out_rows, int mode, void *stream);
int rc_sharded_pages_set(rc_sharded *h, int slot, const int32_t *pages_host, int n_pages);
int rc_sharded_search_pages(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k,
                            const uint32_t *mask, float *scores, int64_t *out_rows, void *stream);
int rc_sharded_search_pages_ex(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k,
                               const uint32_t *mask, float *scores, int64_t *out_rows, int mode, void *stream);
/* rc_sharded_query_host_masked over a slot: host in, host out, one H2D copy, the paged
 * search, the matched positions' values (gathered through the table), one D2H copy,
 * one synchronisation.  out_rows are positions. */
int rc_sharded_query_host_pages(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k,
                                int with_values, const uint32_t *mask, float *scores, int64_t *out_rows,
                                float *values);

/* ------------------------------------------------------------------------
 * Deep top-k: exact results past RC_TOPK_MAX per query, up to RC_DEEP_TOPK_MAX
 * ("Deep top-k").  The calls above keep refusing k > RC_TOPK_MAX; these
 * take 1 <= k <= RC_DEEP_TOPK_MAX and a mask that may be NULL, on every dtype, metric
 * and filter kind (they never run the filter GEMM).
 *
 * One pass over the stored rows writes every row's f32 score (the scan's own bits)
 * to a workspace; ceil(k / RC_TOPK_MAX) selection rounds over those 4 bytes per row
 * follow, round j taking the RC_TOPK_MAX smallest keys at or above a bound that round
 * j - 1 left in device memory (its last key + 1), so all rounds are enqueued at once
 * and nothing waits for the host.  The key is the searches' total order (score
 * descending, then row ascending), so for every k the result is what an exact scan
 * able to hold k keys would give: the first min(k, RC_TOPK_MAX) slots are
 * bit-identical to rc_*_search_masked(..., RC_SEARCH_SCAN) with the same arguments,
 * and slots past the eligible rows are (-inf, -1).  Several shards each select their
 * own k and the leader runs the same rounds over the S x k gathered keys: the result
 * of one index holding the same rows.
 *
 * Masks, rows and positions follow the twins: rc_index_search_deep takes a DEVICE
 * bitmap over the local rows and rc_index_search_pages_deep one over the positions
 * (as rc_index_search_masked / rc_index_search_pages); the rc_sharded_* calls take a
 * HOST bitmap over the global rows / positions.  Queries are processed in chunks of at
 * most RC_DEEP_CHUNK_QUERIES whose scores fit RC_DEEP_WS_BYTES (at least one query);
 * the workspace (4 x local rows bytes per query in flight, the blocks' partial lists
 * and k keys per query of a chunk) is allocated by the first deep call of a size and
 * reused: a repeated call leaves rc_alloc_count() unchanged.  Every argument is
 * checked before any device call (RC_ERR_INVALID).
 *
 * rc_index_scores / rc_index_scores_pages are diagnostics in the style of
 * rc_index_filter_scores: the score pass alone, out_scores (device f32 [n_rows] /
 * [n_pos]) = the score of one raw query against every local row / position. */
#define RC_DEEP_TOPK_MAX 10000
#define RC_DEEP_SELECT_ROWS 2048            /* a selection block owns at least this many stream entries */
#define RC_DEEP_CHUNK_QUERIES 64            /* queries in flight, at most */
#define RC_DEEP_WS_BYTES (256ll << 20)      /* ... and their score arrays, at most (one query always runs) */
int rc_index_search_deep(rc_index *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask,
                         float *scores, int64_t *out_rows, void *stream);
int rc_index_search_pages_deep(rc_index *h, const float *queries, int nq, int slot, int64_t n_pos, int k,
                               const uint32_t *mask, float *scores, int64_t *out_rows, void *stream);
int rc_sharded_search_deep(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask,
                           float *scores, int64_t *out_rows, void *stream);
int rc_sharded_search_pages_deep(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k,
                                 const uint32_t *mask, float *scores, int64_t *out_rows, void *stream);
int rc_index_scores(rc_index *h, const float *query, int64_t n_rows, float *out_scores, void *stream);
int rc_index_scores_pages(rc_index *h, const float *query, int slot, int64_t n_pos, float *out_scores, void *stream);

/* ------------------------------------------------------------------------
 * Sparse-dense hybrid scores on a dotproduct index ("Sparse-dense
 * hybrid"): a record may carry sparse values beside its dense vector, a query a
 * sparse vector, and the score is  dense . dense + sparse . sparse.
 *
 * The store, one per rc_index (per shard), is made by rc_index_sparse_enable(h,
 * width), 1 <= width <= RC_SPARSE_MAX_NNZ: width slots of (uint32 index, f32 value)
 * per local row, slot-major ([width][capacity]: 8 x width x capacity bytes), a row's
 * slots ascending by index, unused ones padded with index 0xFFFFFFFF, which no record
 * or query may carry.  It grows with rc_index_grow and is freed with the index.
 * rc_index_sparse_write takes n local rows as HOST CSR (row rows[i] holds entries
 * [off[i], off[i + 1]) of idx / val: strictly ascending indices, finite values, at
 * most width of them), stages it itself and overwrites ALL width slots of every
 * named row, so a reused row keeps nothing of its former owner; it returns when the
 * store is written.  rc_sharded_sparse_enable / rc_sharded_sparse_write do the same
 * for global rows (shard row % S, local row row / S).  There is no move call: the
 * host layer keeps each id's sparse values and re-writes the rows a compaction moved.
 *
 * The rc_*_search_hybrid calls are their rc_*_search_deep twins plus the sparse
 * queries as HOST CSR: sq_off int32 [nq + 1] from 0, query q holding entries
 * [sq_off[q], sq_off[q + 1]) of sq_idx / sq_val, strictly ascending, at most
 * RC_SPARSE_MAX_NNZ.  They run the deep search with one kernel between its score pass
 * and its selection.  With d the f32 the score pass gives a row (rc_index_scores' bits),
 *   t = +0.0f;  for the row's stored entries (i, v) in ascending i with (i, w) in the
 *   query:  t = fadd(t, fmul(v, w))   (round to nearest, unfused);   score = fadd(d, t).
 * A row without stored entries, and every row under a query without entries, keeps
 * d's bits: with no sparse entries at all the call is rc_*_search_deep bit for bit.
 * The result is the first k keys of the searches' total order (score descending, row
 * ascending) over the eligible rows, for 1 <= k <= RC_DEEP_TOPK_MAX.  Masks, rows,
 * positions, chunking and workspace follow the deep calls (a repeated call leaves
 * rc_alloc_count() unchanged).  Every argument is checked before any device call
 * (RC_ERR_INVALID): a store that is not enabled, a metric other than
 * RC_METRIC_DOT, unsorted or repeated query indices, more than RC_SPARSE_MAX_NNZ
 * entries, the padding value as an index, k outside [1, RC_DEEP_TOPK_MAX].
 *
 * rc_index_scores_hybrid is a diagnostic: rc_index_scores (slot < 0) or
 * rc_index_scores_pages (slot >= 0) plus the add, for one query (sq_off [2]). */
#define RC_SPARSE_MAX_NNZ 1024
int rc_index_sparse_enable(rc_index *h, int width, void *stream);
int rc_index_sparse_width(const rc_index *h, int *width); /* 0: not enabled */
int rc_index_sparse_write(rc_index *h, const int64_t *rows, const int64_t *off, const uint32_t *idx, const float *val,
                          int64_t n, void *stream);
int rc_sharded_sparse_enable(rc_sharded *h, int width);
int rc_sharded_sparse_write(rc_sharded *h, const int64_t *rows, const int64_t *off, const uint32_t *idx, const float *val,
                            int64_t n);
int rc_index_search_hybrid(rc_index *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask,
                           const int32_t *sq_off, const uint32_t *sq_idx, const float *sq_val, float *scores,
                           int64_t *out_rows, void *stream);
int rc_index_search_pages_hybrid(rc_index *h, const float *queries, int nq, int slot, int64_t n_pos, int k,
                                 const uint32_t *mask, const int32_t *sq_off, const uint32_t *sq_idx, const float *sq_val,
                                 float *scores, int64_t *out_rows, void *stream);
int rc_sharded_search_hybrid(rc_sharded *h, const float *queries, int nq, int64_t n_rows, int k, const uint32_t *mask,
                             const int32_t *sq_off, const uint32_t *sq_idx, const float *sq_val, float *scores,
                             int64_t *out_rows, void *stream);
int rc_sharded_search_pages_hybrid(rc_sharded *h, const float *queries, int nq, int slot, int64_t n_pos, int k,
                                   const uint32_t *mask, const int32_t *sq_off, const uint32_t *sq_idx, const float *sq_val,
                                   float *scores, int64_t *out_rows, void *stream);
int rc_index_scores_hybrid(rc_index *h, const float *query, int slot, int64_t n, const int32_t *sq_off,
                           const uint32_t *sq_idx, const float *sq_val, float *out_scores, void *stream);

/* ------------------------------------------------------------------------
 * Metadata columns: the indexed metadata fields of an index's rows as typed
 * columns in device memory, and the kernel that turns a metadata filter
 * (index.query(filter=...)) into the row-eligibility bitmap the masked searches
 * take.  Stateless: the caller owns every buffer (the host layer keeps them as
 * torch tensors) and the three calls only enqueue work on `stream`.
 *
 * Layout, F = n_fields fields over `capacity` rows, field-major:
 *   tags  uint8 [F, capacity]   RC_META_TAG_* of field f of row r at tags[f * capacity + r]
 *   vals  int64 [F, capacity]   NUMBER: the float64 bits; BOOL: 0 / 1; STRING: the string's
 *                               code in the host's dictionary of that field; ABSENT: unused
 *
 * rc_meta_write scatters n rows: field f of device row rows[i] becomes
 * (in_tags[f * n + i], in_vals[f * n + i]) for EVERY f, so a reused row keeps nothing
 * of its former owner.  rows must be distinct.  rc_meta_move copies all fields of row
 * src_rows[i] to row dst_rows[i] (the two lists disjoint, as rc_index_move_rows).
 * rows, src_rows, dst_rows, in_tags and in_vals are DEVICE buffers; a row outside
 * [0, capacity) is skipped by the kernel, never written.
 *
 * rc_meta_eval evaluates a postfix program at positions [0, n) and writes
 * out_words uint32 [ceil(n / 32)] (bit p & 31 of word p >> 5 = position p satisfies the
 * program; bits at or past n clear — rc_index_search_masked's layout) and *out_count
 * (how many do), both DEVICE buffers.  Without a page list position p is row p; with
 * one (pages_host, HOST int32 [n_pages], span a multiple of 256) it is row
 * pages[p / span] * span + p % span: a namespace's page list over the pool's global
 * rows, span = RC_PAGE_ROWS * shards.
 *
 * The program is HOST int64 [2 * n_instr], two words per instruction:
 *   word 0 = op | field << 8 | operand tag << 16 | k << 32,  word 1 = operand val.
 * A leaf (RC_META_EQ .. RC_META_NOT_EXISTS) pushes one boolean computed from field
 * `field` of the row and the operand; RC_META_TRUE / RC_META_FALSE push a constant;
 * RC_META_AND / RC_META_OR replace the top k entries by their conjunction /
 * disjunction.  The result is the one entry left at the end.  Comparison rules:
 *   EQ   the tags are equal and the values are: NUMBER compares as IEEE float64 (so
 *        -0.0 equals 0.0 and a NaN equals nothing, itself included), BOOL and STRING as
 *        integers.  An absent field equals nothing.  NE is the negation of EQ.
 *   GT GE LT LE   both tags are NUMBER and the float64 comparison holds; else false.
 *   EXISTS / NOT_EXISTS   the row's tag is not / is RC_META_TAG_ABSENT.
 * Limits: n_fields <= RC_META_MAX_FIELDS, n_instr <= RC_META_MAX_INSTR, stack depth
 * <= RC_META_MAX_STACK (the lane's stack is one 64-bit register).
 *
 * workspace: DEVICE scratch of at least 16 * n_instr + 4 * n_pages bytes, 16-byte
 * aligned; the call uploads the checked program and page list there.  program_host and
 * pages_host must stay valid until `stream` has passed the call.
 *
 * Every check runs before any device call and returns RC_ERR_INVALID: NULL buffers,
 * n beyond the capacity (or beyond n_pages * span), a page at or past capacity / span,
 * a span that is not a positive multiple of 256, a small or misaligned workspace, and a
 * malformed program (unknown op, field >= n_fields, an operand tag that is no value's,
 * a combinator that takes more entries than the stack holds, a stack deeper than
 * RC_META_MAX_STACK, anything but one entry left).  A program that passes cannot make
 * the kernel read outside the columns. */
#define RC_META_TAG_ABSENT 0
#define RC_META_TAG_NUMBER 1
#define RC_META_TAG_BOOL 2
#define RC_META_TAG_STRING 3
#define RC_META_EQ 0
#define RC_META_NE 1
#define RC_META_GT 2
#define RC_META_GE 3
#define RC_META_LT 4
#define RC_META_LE 5
#define RC_META_EXISTS 6
#define RC_META_NOT_EXISTS 7
#define RC_META_TRUE 8
#define RC_META_FALSE 9
#define RC_META_AND 10
#define RC_META_OR 11
#define RC_META_MAX_FIELDS 64
#define RC_META_MAX_INSTR 512
#define RC_META_MAX_STACK 64
int rc_meta_write(uint8_t *tags, int64_t *vals, int n_fields, int64_t capacity, const int64_t *rows,
                  const uint8_t *in_tags, const int64_t *in_vals, int64_t n, void *stream);
int rc_meta_move(uint8_t *tags, int64_t *vals, int n_fields, int64_t capacity, const int64_t *src_rows,
                 const int64_t *dst_rows, int64_t n, void *stream);
int rc_meta_eval(const uint8_t *tags, const int64_t *vals, int n_fields, int64_t capacity,
                 const int64_t *program_host, int n_instr, const int32_t *pages_host, int n_pages, int span,
                 int64_t n, void *workspace, int64_t workspace_bytes, uint32_t *out_words, uint32_t *out_count,
                 void *stream);

/* ------------------------------------------------------------------------
 * ViT-MSN image embedding.  Replaces the /embed compute path —
 * embedding/main.py:97-114: PIL decode (stays on host) → ViTImageProcessor
 * (resize, rescale, normalize) → ViTMSNModel → last_hidden_state[:, 0, :].
 * ---------------------------------------------------------------------- */
typedef struct rc_vit_config {
    int image_size;   /* 224 */
    int patch;        /* 16 */
    int hidden;       /* 768 */
    int layers;       /* 12 */
    int heads;        /* 12 */
    int mlp;          /* 3072 */
    float ln_eps;     /* 1e-6 */
    int max_batch;    /* workspace is sized for this many images per rc_embed call */
} rc_vit_config;

/* replaces ViTMSNModel.from_pretrained(...).to(DEVICE) — embedding/main.py:37-39 */
int rc_model_create(int device, const rc_vit_config *cfg, rc_model **out);
int rc_model_destroy(rc_model *m);
/* One state-dict tensor by checkpoint key (legacy layout, e.g.
 * "encoder.layer.3.attention.attention.query.weight"; an optional "vit."
 * prefix and the transformers-5 names "layers.N.attention.q_proj.weight" are
 * also accepted).  host_data: host f32, numel must match. */
int rc_model_set_weight(rc_model *m, const char *name, const float *host_data, int64_t numel);
/* Preprocessor parameters (ViTImageProcessor: resample, rescale_factor, image_mean, image_std). */
int rc_model_set_preprocess(rc_model *m, int resample, double rescale_factor, const float mean[3], const float std_[3]);
/* Verify every weight was set and build the fused device layouts. */
int rc_model_finalize(rc_model *m);

/* replaces embedding/main.py:107-114 for a batch.
 * images: device u8 [n, h, w, 3] (HWC RGB, as decoded by PIL); n <= max_batch.
 * (h, w) != (image_size, image_size) → Pillow-exact resize on the device first.
 * raw_out: device f32 [n, hidden] = last_hidden_state[:, 0, :] (the /embed body);
 * normed_out: device f32 [n, hidden] L2-normalised copy for the index (may be NULL). */
int rc_embed(rc_model *m, const uint8_t *images, int n, int h, int w,
             float *raw_out, float *normed_out, void *stream);

/* Preprocess only: device u8 [n,h,w,3] → device f32 pixel_values [n,3,S,S]
 * exactly as ViTImageProcessor produces them (for parity tests). */
int rc_preprocess(rc_model *m, const uint8_t *images, int n, int h, int w, float *pixel_values, void *stream);

/* Encode a batch as `parts` (1..4) concurrent slices on their own HIP streams
 * (default 2; slices below 32 images are merged).  Results are bit-identical
 * for every setting: each image's arithmetic is the same.  One slice's memory-
 * bound kernels (LayerNorm, attention) and GEMM store bursts then overlap the
 * other slices' MFMA main loops.  rc_embed still returns ordered on `stream`. */
int rc_model_set_parts(rc_model *m, int parts);

/* Last encoder layer on the CLS rows only (default 1).  /embed returns
 * last_hidden_state[:, 0, :] (embedding/main.py:113-114), and row 0 of the last
 * layer (modeling_vit_msn.py:254-283) reads only its own query row plus every
 * token's K/V: with cls_only = 1 the last layer runs LN1 + QKV on all rows, then
 * CLS-query attention, O-proj, LN2 and the MLP on the CLS rows alone.
 * cls_only = 0 runs the whole layer (A/B and parity tests). */
int rc_model_set_last_layer(rc_model *m, int cls_only);

/* LayerNorm fold (default 1): the two LayerNorms of each layer
 * (modeling_vit_msn.py:258-259) are folded into the GEMMs around them — the residual producers (patch embed, O-proj, fc2) also
 * write bf16(x) and per-256-column (mean, M2) partials, and QKV / fc1 apply
 * rstd·(x·(W∘γ)ᵀ − μ·Σ_k W∘γ) + (b + W·β) in their epilogues — instead of a
 * standalone LayerNorm pass over the f32 stream.  0 runs the LN kernel (A/B and
 * parity tests). */
int rc_model_set_ln_fold(rc_model *m, int on);

/* QKV projection fused into attention (default 1 = auto).  For the model's real shape (197
 * tokens, hidden 768, 12 heads, LayerNorm fold on) one kernel computes a head's Q, K and V
 * from the residual rows into LDS and runs attention there, so the qkv tensor never goes
 * through HBM.  Same bits as the two kernels it replaces.  0 = off; 1 = for the batch
 * parts where it measured faster; 2 = whenever the shape qualifies, at any batch size.
 * Other shapes, and the CLS-only last layer, always run the separate kernels. */
int rc_model_set_qkv_fusion(rc_model *m, int mode);

/* Batch-1 HIP graphs (default 1): an rc_embed of one image at the model's input size
 * (the reference's /embed request, embedding/main.py:88-124) replays a HIP graph of its
 * launch chain, captured on first use per (images, raw_out, normed_out) buffer triple
 * (at most 8 kept, least recently used evicted; after 8 misses in a row only a triple that
 * misses twice in a row is captured, the others run the stream form): one host launch per
 * request instead of ~70.  Same kernels, same bits.  Every setter drops the captured graphs.
 * 0 = stream form. */
int rc_model_set_graphs(rc_model *m, int on);

/* Per-kernel timing with HIP events on the launch stream (bench/roofline).
 * kernel ids: 0 = all GEMMs, 1 = fc1 GEMM, 2 = attention, 3 = layernorm,
 * 4 = preprocess, 5 = QKV GEMM, 6 = O-proj GEMM, 7 = fc2 GEMM (5-7 and 1: the
 * full-batch launches of that projection); `mask` bit i enables id i (-1 = all, 0 = off). */
int rc_model_timing(rc_model *m, int mask);
int rc_model_timing_read(rc_model *m, int kernel_id, double *total_ms, int64_t *launches, double *flops);
int rc_model_timing_reset(rc_model *m);

/* Kernel-level entry to the projection GEMM (parity tests / microbenchmarks;
 * inside rc_embed this is every nn.Linear of modeling_vit_msn.py:199-202,243-244).
 * out = epilogue(A[M][K] · W[N][K]ᵀ + bias): epi 0 → bf16 out, 1 → bf16 GELU(out),
 * 2 → f32 out += (residual, in place), 3 → f32 patch scatter (+pos, tokens/image).
 * A must have round_up(M, 256) readable rows; N % 256 == 0 (M > 256), K % 64 == 0.
 * variant: 0 auto, 4 256x256 ping-pong, 8 128x256 two-workgroup, 9 skinny (M <= 256),
 * 10 image-aligned 224-row tiles (the model's O-proj / fc2 kernel; epi 2 only, `tokens` =
 * rows per image, tile t = rows [t·tokens, t·tokens + tokens); A must then hold
 * ceil(M / tokens)·tokens + 224 − tokens readable rows). */
int rc_gemm_bf16(int epi, int variant, const uint16_t *A, const uint16_t *W, const float *bias, int M, int N, int K,
                 void *out, const float *pos, int tokens, void *stream);

/* Kernel-level entry to the attention kernels (parity tests; inside rc_embed this is the eager
 * attention of modeling_vit_msn.py:161-186), launched by the launcher the model uses.
 * qkv [images·tokens][3·heads·64] bf16 with Q | K | V columns as the model lays them out, head
 * dim 64, scale log2(e)/8 folded into exp2.  out = softmax(Q·Kᵀ/8)·V per (image, head), bf16.
 * kind 0: full attention as rc_embed launches it (the 197-token instantiation at tokens == 197,
 * the runtime-token-count one otherwise), out [images·tokens][heads·64]; kind 1: the same with
 * the runtime-token-count instantiation at any count; kind 2: the CLS query only (the last
 * layer), out [images][heads·64], the queries from q_cls (compact [images][heads·64]) or, when
 * q_cls is null, from row 0 of each image in qkv.  qsplit (full kinds): blocks per (image,
 * head), 1 or 4, or 0 for the model's choice (4 below one item per compute unit).  tokens:
 * 1 .. 208 (full kinds), 1 .. 256 (kind 2).  Anything else, null qkv / out and images or
 * heads < 1 are RC_ERR_INVALID before any device call.  Pointers must be 16-byte aligned. */
int rc_attention_bf16(int kind, const uint16_t *qkv, const uint16_t *q_cls, uint16_t *out, int images, int tokens,
                      int heads, int qsplit, void *stream);

/* Index-side timing of the dominant search kernel (scan), same conventions. */
int rc_index_timing(rc_index *h, int enable);
int rc_index_timing_read(rc_index *h, double *total_ms, int64_t *launches, double *bytes);
/* Same for the batched search's filter GEMM (flops = 2 * query slots * rows * ld per launch);
 * fallbacks = queries re-run through the on-device exact scan since the last
 * read (candidate overflow; synchronises the device to read the counter). */
int rc_index_gemm_timing_read(rc_index *h, double *total_ms, int64_t *launches, double *flops, int64_t *fallbacks);


/* ------------------------------------------------------------------------
 * JPEG decode.  Replaces Image.open(BytesIO(bytes)).convert("RGB") —
 * embedding/main.py:97 — for baseline JPEGs: Huffman decode on the host
 * (one thread per image), dequantisation + islow IDCT + fancy upsampling +
 * YCbCr->RGB on the GPU, bit-exact with Pillow/libjpeg-turbo defaults.
 * Other streams (progressive, arithmetic, 12-bit, CMYK/RGB colour spaces,
 * multi-scan) report supported = 0 and stay on the host decode path.
 * ---------------------------------------------------------------------- */
typedef struct rc_jpeg_info {
    int32_t width, height, ncomp, supported;
    int32_t hmax, vmax, restart_interval, mcux, mcuy;
    int32_t h[3], v[3];   /* sampling factors per component */
    int32_t bw[3], bh[3]; /* 8x8 blocks per component plane (MCU padded) */
    int64_t blocks;       /* coefficient blocks of the image, all planes */
} rc_jpeg_info;
typedef struct rc_jpeg_decoder rc_jpeg_decoder;

/* Header walk: size, components, sampling, whether rc_jpeg_decode handles it.
 * RC_ERR_INVALID if the bytes are not a JPEG stream (the caller's
 * UnidentifiedImageError path, embedding/main.py:115-119). */
int rc_jpeg_probe(const uint8_t *jpg, int64_t len, rc_jpeg_info *info);
/* Host-only entropy decode (test hook): quantised coefficients of every block,
 * natural order, planes in component order ([blocks][64] int16), and each
 * component's quantisation table in natural order ([ncomp][64] u16). */
int rc_jpeg_decode_coefficients(const uint8_t *jpg, int64_t len, int16_t *coef, uint16_t *qtab);
/* Pinned host staging + device workspace for up to max_images images and
 * max_blocks coefficient blocks per call (no allocation in rc_jpeg_decode). */
int rc_jpeg_decoder_create(int device, int max_images, int64_t max_blocks, rc_jpeg_decoder **out);
int rc_jpeg_decoder_destroy(rc_jpeg_decoder *h);
/* Decode n JPEGs (host buffers) into device HWC RGB u8: image i is written at
 * rgb + rgb_offsets[i] (host array, bytes), height x width x 3.  The host
 * buffers may be reused once the call returns; the reconstruction is ordered
 * on `stream`.  RC_ERR_UNSUPPORTED if any image is outside what the decoder
 * handles (probe first), RC_ERR_INVALID for damaged or truncated data. */
int rc_jpeg_decode(rc_jpeg_decoder *h, int n, const uint8_t *const *jpgs, const int64_t *lens, uint8_t *rgb,
                   const int64_t *rgb_offsets, void *stream);
/* Decode n JPEGs (any sizes, mixed) straight to out_size x out_size: the decode above
 * followed by Pillow's resample (`resample` = RC_RESAMPLE_BICUBIC / _BILINEAR, the
 * ViTImageProcessor resize of embedding/main.py:107), with the colour pass fused into
 * the horizontal resample (the full-size RGB image is never written).  out: device u8
 * [n][out_size][out_size][3], bit-exact with PIL decode + Image.resize.  A horizontal
 * pass buffer grows with the largest batch seen (no allocation once warm). */
int rc_jpeg_decode_resized(rc_jpeg_decoder *h, int n, const uint8_t *const *jpgs, const int64_t *lens, int out_size,
                           int resample, uint8_t *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RETRIEVAL_CORE_H */
