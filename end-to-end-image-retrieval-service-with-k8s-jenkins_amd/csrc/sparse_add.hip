// sparse_add.hip — the sparse half of a sparse-dense hybrid score (sparse.h; DESIGN.md,
// "Sparse-dense hybrid"): the kernel that adds each row's sparse term to the f32 score the deep
// top-k's score pass wrote, the store's scatter write and its regrow, and the host staging of the
// sparse queries.  Nothing here reads a dense row.
#include "sparse.h"

#include <algorithm>
#include <cmath>

namespace rc {

namespace {

constexpr int SPARSE_ADD_ROWS = 1024;  // rows (positions) a block walks, 256 at a time: the query is staged once for them

// t + v * w as two roundings.  hipcc contracts a * b + c into one fma by default, and __fmul_rn /
// __fadd_rn are plain operators to it, so the contraction is switched off where the term is formed.
__device__ __forceinline__ float add_product(float t, float v, float w) {
#pragma clang fp contract(off)
    const float p = v * w;
    return t + p;
}

// One lane owns one row: it walks the row's slots in ascending index order (slot-major store, so a
// wave's loads of slot j are consecutive dwords), looks each index up in the query's sorted pairs
// in LDS — a lower bound from where the last one ended, both lists ascend — and accumulates
//   t = fadd(t, fmul(v, w)), unfused (add_product), from +0.0f,
// then adds t to the row's score.  A wave stops at the first slot that is padding in all its lanes.
// grid = (row blocks, queries); a query without entries exits at once and a row whose first slot
// is padding is not written, so both keep the score pass's bits.
template <bool PAGED>
__global__ __launch_bounds__(256) void sparse_add_kernel(const uint32_t *__restrict__ s_idx, const float *__restrict__ s_val, int width,
                                                        int64_t capacity, const int32_t *__restrict__ q_off,
                                                        const uint32_t *__restrict__ q_idx, const float *__restrict__ q_val, int q0,
                                                        int64_t n, const int32_t *__restrict__ pages, float *__restrict__ scores) {
    __shared__ uint32_t qi[RC_SPARSE_MAX_NNZ];
    __shared__ float qv[RC_SPARSE_MAX_NNZ];
    const int q = blockIdx.y;
    const int b = q_off[q0 + q];
    const int qn = min(q_off[q0 + q + 1] - b, RC_SPARSE_MAX_NNZ);  // (the host checked it: never cut)
    if (qn <= 0) return;
    for (int i = threadIdx.x; i < qn; i += 256) {
        qi[i] = q_idx[b + i];
        qv[i] = q_val[b + i];
    }
    __syncthreads();
    float *sc = scores + (int64_t)q * n;
    const int64_t first = (int64_t)blockIdx.x * SPARSE_ADD_ROWS;
    const int64_t last = min(n, first + SPARSE_ADD_ROWS);
    for (int64_t base = first; base < last; base += 256) {  // block-uniform trip count: the ballots below see whole waves
        const int64_t r = base + threadIdx.x;
        const bool live = r < n;
        int64_t row = 0;
        if (live) row = PAGED ? (int64_t)pages[r / RC_PAGE_ROWS] * RC_PAGE_ROWS + r % RC_PAGE_ROWS : r;
        float t = 0.0f;
        bool any = false;
        int lo = 0;
        for (int j = 0; j < width; ++j) {
            const uint32_t ix = live ? s_idx[(int64_t)j * capacity + row] : SPARSE_PAD;
            if (__ballot(ix != SPARSE_PAD) == 0ull) break;
            if (ix != SPARSE_PAD) {
                any = true;
                int hi = qn;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (qi[mid] < ix) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < qn && qi[lo] == ix) {
                    t = add_product(t, s_val[(int64_t)j * capacity + row], qv[lo]);
                    ++lo;
                }
            }
        }
        if (any) sc[r] = __fadd_rn(sc[r], t);
    }
}

// entry e = (i, j) of a row-major block [n][width]: slot j of row rows[i]
__global__ __launch_bounds__(256) void sparse_scatter_kernel(uint32_t *__restrict__ s_idx, float *__restrict__ s_val, int width,
                                                            int64_t capacity, const int64_t *__restrict__ rows,
                                                            const uint32_t *__restrict__ in_idx, const float *__restrict__ in_val,
                                                            int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * width) return;
    const int64_t row = rows[e / width];
    if (row < 0 || row >= capacity) return;
    const int64_t at = (e % width) * capacity + row;
    s_idx[at] = in_idx[e];
    s_val[at] = in_val[e];
}

__global__ __launch_bounds__(256) void sparse_regrow_kernel(const uint32_t *__restrict__ o_idx, const float *__restrict__ o_val,
                                                           int64_t old_cap, uint32_t *__restrict__ idx, float *__restrict__ val,
                                                           int64_t new_cap, int64_t total) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t j = e / new_cap, r = e % new_cap;
        const bool old = r < old_cap;
        idx[e] = old ? o_idx[j * old_cap + r] : SPARSE_PAD;
        val[e] = old ? o_val[j * old_cap + r] : 0.0f;
    }
}

// a pinned block and its device twin, replaced by larger ones
template <typename T>
void realloc_pair(T *&h, T *&d, size_t count) {
    hfree(h);
    dfree(d);
    h = nullptr;
    d = nullptr;
    h = (T *)hmalloc(count * sizeof(T));
    d = (T *)dmalloc(count * sizeof(T));
}

}  // namespace

void sparse_check_queries(const SparseQueries &sq, int nq) {
    RC_REQUIRE(sq.off != nullptr, RC_ERR_INVALID, "null sparse query offsets");
    RC_REQUIRE(sq.off[0] == 0, RC_ERR_INVALID, "sparse query offsets must start at 0");
    for (int q = 0; q < nq; ++q) {
        const int32_t b = sq.off[q], e = sq.off[q + 1];
        RC_REQUIRE(e >= b, RC_ERR_INVALID, "sparse query offsets must not descend");
        RC_REQUIRE(e - b <= RC_SPARSE_MAX_NNZ, RC_ERR_INVALID, "a sparse query holds at most 1024 entries");
        RC_REQUIRE(e == b || (sq.idx != nullptr && sq.val != nullptr), RC_ERR_INVALID, "null sparse query entries");
        for (int32_t i = b; i < e; ++i) {
            RC_REQUIRE(sq.idx[i] != SPARSE_PAD, RC_ERR_INVALID, "sparse index 2^32 - 1 is reserved (the store's padding)");
            RC_REQUIRE(i == b || sq.idx[i] > sq.idx[i - 1], RC_ERR_INVALID, "sparse query indices must be strictly ascending");
            RC_REQUIRE(std::isfinite(sq.val[i]), RC_ERR_INVALID, "sparse query values must be finite");
        }
    }
}

void SparseWs::wait() {
    if (pending) RC_HIP(hipEventSynchronize(ev));
    pending = false;
}

void SparseWs::stage_queries(const SparseQueries &sq, int nq, hipStream_t s) {
    const int64_t total = sq.off[nq];
    if (ev == nullptr) RC_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    wait();
    if (nq + 1 > off_cap) {
        off_cap = 0;
        realloc_pair(off_h, off_d, (size_t)nq + 1);
        off_cap = nq + 1;
    }
    if (total > q_cap) {
        const int64_t c2 = std::max<int64_t>(total, 2 * q_cap);
        q_cap = 0;
        realloc_pair(idx_h, idx_d, (size_t)c2);
        realloc_pair(val_h, val_d, (size_t)c2);
        q_cap = c2;
    }
    std::memcpy(off_h, sq.off, ((size_t)nq + 1) * sizeof(int32_t));
    RC_HIP(hipMemcpyAsync(off_d, off_h, ((size_t)nq + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (total > 0) {
        std::memcpy(idx_h, sq.idx, (size_t)total * sizeof(uint32_t));
        std::memcpy(val_h, sq.val, (size_t)total * sizeof(float));
        RC_HIP(hipMemcpyAsync(idx_d, idx_h, (size_t)total * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        RC_HIP(hipMemcpyAsync(val_d, val_h, (size_t)total * sizeof(float), hipMemcpyHostToDevice, s));
    }
    RC_HIP(hipEventRecord(ev, s));
    pending = true;
}

void SparseWs::ensure_write(int64_t rows, int width) {
    if (ev == nullptr) RC_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    if (rows > w_rows) {
        w_rows = 0;
        realloc_pair(wrow_h, wrow_d, (size_t)rows);
        w_rows = rows;
    }
    const int64_t slots = rows * width;
    if (slots > w_slots) {
        w_slots = 0;
        realloc_pair(widx_h, widx_d, (size_t)slots);
        realloc_pair(wval_h, wval_d, (size_t)slots);
        w_slots = slots;
    }
}

void SparseWs::release() {
    for (void *p : {(void *)off_h, (void *)idx_h, (void *)val_h, (void *)wrow_h, (void *)widx_h, (void *)wval_h}) hfree(p);
    for (void *p : {(void *)off_d, (void *)idx_d, (void *)val_d, (void *)wrow_d, (void *)widx_d, (void *)wval_d}) dfree(p);
    if (ev != nullptr) (void)hipEventDestroy(ev);
    *this = SparseWs{};
}

void launch_sparse_add(const SparseAddArgs &a) {
    if (a.nq <= 0 || a.n <= 0) return;
    const dim3 grid((unsigned)((a.n + SPARSE_ADD_ROWS - 1) / SPARSE_ADD_ROWS), (unsigned)a.nq);
    if (a.pages != nullptr)
        hipLaunchKernelGGL(sparse_add_kernel<true>, grid, dim3(256), 0, a.stream, a.s_idx, a.s_val, a.width, a.capacity, a.q_off,
                           a.q_idx, a.q_val, a.q0, a.n, a.pages, a.scores);
    else
        hipLaunchKernelGGL(sparse_add_kernel<false>, grid, dim3(256), 0, a.stream, a.s_idx, a.s_val, a.width, a.capacity, a.q_off,
                           a.q_idx, a.q_val, a.q0, a.n, a.pages, a.scores);
    RC_LAUNCH_CHECK();
}

void launch_sparse_scatter(const SparseStore &st, int64_t capacity, const int64_t *rows, const uint32_t *in_idx, const float *in_val,
                           int64_t n, hipStream_t s) {
    if (n <= 0) return;
    const int64_t total = n * st.width;
    hipLaunchKernelGGL(sparse_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, st.idx, st.val, st.width, capacity,
                       rows, in_idx, in_val, n);
    RC_LAUNCH_CHECK();
}

void launch_sparse_regrow(const SparseStore &from, int64_t old_cap, uint32_t *idx, float *val, int64_t new_cap, hipStream_t s) {
    const int64_t total = (int64_t)from.width * new_cap;
    const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(sparse_regrow_kernel, dim3(grid), dim3(256), 0, s, from.idx, from.val, old_cap, idx, val, new_cap, total);
    RC_LAUNCH_CHECK();
}

}  // namespace rc
