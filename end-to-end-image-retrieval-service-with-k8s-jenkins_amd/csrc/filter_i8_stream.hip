// filter_i8_stream.hip — the int8 filter for 1 to 8 queries (RC_FILTER_I8_STREAM): an HBM-bound
// stream over the index's int8 copy in place of the 256-query MFMA tile of filter_i8_kernel.
//
// Exactness: the kernel applies filter_i8_kernel's keep rule, sq·(sx·D) + ex·aq >= thr[q], to the same
// exact integer D and the same sx, ex, sq, aq, thr, so search_mfma.hip's "int8 filter" proof carries over.
//
// Work split.  A block of 4 waves walks row tiles of 128 rows, `tiles_per_chunk` of them in a row
// (persistent: a stage is one launch).  Inside a tile a group of 16 lanes owns the 8 rows 16·u + li,
// li = 4·wave + lane / 16, which are the 8 consecutive floats li·8 .. li·8 + 7 of the tile's sx / ex
// (i8_slot): one vector load each per step.  A step is U of those rows; a lane reads the 16-byte chunks
// sub + 16·i (sub = lane % 16, i < LD / 256) of each, so one load instruction of a wave covers four
// consecutive rows' 256-byte segments, and a block's tile is LD·128 consecutive bytes.
// Nothing passes through LDS: the rows go from nontemporal global loads to the dot instruction.  Two
// register buffers alternate, the next step's loads issued before the current step is consumed:
// 8 row loads in flight per lane at ld 256 and 512 (what the exact scan keeps for f16 rows), 12 at 768.
// The NQ queries' int8 chunks for a lane's columns stay in registers for the whole kernel
// (NQ · LD / 64 dwords), so the loop reads row bytes, sx and ex only.
// D = q8·x8 accumulates in v_dot4c_i32_i8 (exact in i32), is summed over the 16 lanes of the row by four
// DPP row steps (integer adds: any order gives the same sum), after which lane sub < NQ of the group
// holds query sub's D and forms u with the arithmetic and operand order of filter_i8_kernel's keep test.
// Appends go to a per-block LDS list of I8S_SL rows per query (LDS atomics wait on lgkmcnt alone; a
// returning global atomic would wait for every row load in flight) flushed with one global atomic per
// query at the block's end; a full list falls through to append_candidate.  The global count keeps
// running past cap, which is what rescore_kernel reads an overflow from.
// DUMP (rc_index_filter_scores): u itself is stored instead of tested; the loads, the dot and the
// reduction are the product's.
#include <algorithm>

#include "filter_mfma.h"

namespace rc {

constexpr int I8S_TILE = 128;  // rows per tile: one i8_slot tile
constexpr int I8S_SL = 24;     // candidate rows staged in LDS per query per block
constexpr int I8S_CUS = 256;   // compute units a stage is spread over

// rows of a 16-lane group per step: 2 buffers x U x LD / 256 loads in flight
constexpr int i8s_u(int ld) { return ld == 256 ? 4 : 2; }
// blocks per compute unit the grid is sized for: 4 where the kernel's registers let 4 waves share a SIMD
// (up to 16 query dwords per lane, NQ · LD / 64; every instantiation fits 2), so that the whole grid is resident
constexpr int i8s_bpc(int ld, int nq) { return nq * ld / 64 <= 16 ? 4 : 2; }

struct FilterI8StreamArgs {
    FilterArgs a;  // rows: the int8 copy; qh: q8 [8][ld]; r_begin a multiple of 128; tiles of I8S_TILE rows; nqb unused
    float *dump;   // DUMP: u of queries [0, dump_nq) x rows [r_begin, r_end), [dump_nq][r_end - r_begin]
    int dump_nq;
};

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
// sum16 (rc_common.h) over integers: every lane of an aligned group of 16 gets the group's sum
__device__ __forceinline__ int sum16_i32(int v) {
    v += dpp_i32<0xB1>(v);
    v += dpp_i32<0x4E>(v);
    v += dpp_i32<0x141>(v);
    v += dpp_i32<0x140>(v);
    return v;
}

template <int LD, int NQ, bool DUMP = false>
__global__ __launch_bounds__(256) void filter_i8_stream_kernel(FilterI8StreamArgs fa) {
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    typedef float f32xu_t __attribute__((ext_vector_type(i8s_u(LD))));
    constexpr int CPL = LD / 256, U = i8s_u(LD), SPT = 8 / U;
    static_assert((LD == 256 || LD == 512 || LD == 768) && (NQ == 1 || NQ == 2 || NQ == 4 || NQ == 8), "instantiated shapes");
    const FilterArgs &a = fa.a;
    __shared__ uint32_t lcnt[NQ];
    __shared__ uint32_t lbuf[NQ][I8S_SL];

    const int tid = threadIdx.x, lane = tid & 63;
    const int sub = lane & 15, li = (tid >> 6) * 4 + (lane >> 4);
    const int64_t nt = (a.r_end - a.r_begin + I8S_TILE - 1) / I8S_TILE;
    const int64_t t0 = (int64_t)blockIdx.x * a.tiles_per_chunk, t1 = min(nt, t0 + a.tiles_per_chunk);
    if (t0 >= t1) return;  // block-uniform
    if (tid < NQ) lcnt[tid] = 0u;
    __syncthreads();

    // the lane's columns of every query, and the constants of the query it tests (lanes sub >= NQ test none)
    int qr[NQ][CPL][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const i32x4_t v = *reinterpret_cast<const i32x4_t *>((const int8_t *)a.qh + q * LD + (sub + 16 * i) * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) qr[q][i][j] = v[j];
        }
    const int qme = sub & (NQ - 1);
    const bool tester = DUMP ? sub < fa.dump_nq && sub < NQ : sub < NQ;
    const float thr = a.thr[qme], sq = a.sq[qme], aq = a.aq[qme];

    struct Step {
        i32x4_t x[U][CPL];
        f32xu_t sx, ex;
    };
    // step s of the block: rows tile·128 + 16·(part·U + u) + li, u < U.  A row at or past r_end is
    // read as row r_end - 1 (inside the copy whatever its padding) and never appended.
    auto issue = [&](int64_t s, Step &b) __attribute__((always_inline)) {
        const int64_t tile = s / SPT;
        const int part = (int)(s - tile * SPT);
        const int64_t tb = a.r_begin + tile * I8S_TILE;  // a multiple of 128: the tile's i8_slot base
        const int last = (int)min<int64_t>(I8S_TILE - 1, a.r_end - 1 - tb);
        const int8_t *base = (const int8_t *)a.rows + tb * LD;
        b.sx = *reinterpret_cast<const f32xu_t *>(a.rsx + tb + li * 8 + part * U);
        b.ex = *reinterpret_cast<const f32xu_t *>(a.rex + tb + li * 8 + part * U);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = min(16 * (part * U + u) + li, last);
#pragma unroll
            for (int i = 0; i < CPL; ++i)
                b.x[u][i] = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t *>(base + r * LD + (sub + 16 * i) * 16));
        }
    };
    auto consume = [&](int64_t s, const Step &b) __attribute__((always_inline)) {
        const int64_t tile = s / SPT;
        const int part = (int)(s - tile * SPT);
        const int64_t row0 = a.r_begin + tile * I8S_TILE + 16 * part * U + li;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int d = 0;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                int acc = 0;
#pragma unroll
                for (int i = 0; i < CPL; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_sdot4(b.x[u][i][j], qr[q][i][j], acc, false);
                acc = sum16_i32(acc);
                d = q == 0 || qme == q ? acc : d;
            }
            const int64_t row = row0 + 16 * u;
            const float v = fmaf(b.ex[u], aq, sq * (b.sx[u] * (float)d));
            if constexpr (DUMP) {
                if (tester && row < a.r_end) fa.dump[(int64_t)qme * (a.r_end - a.r_begin) + (row - a.r_begin)] = v;
            } else if (tester && v >= thr && row < a.r_end) {
                const uint32_t p = atomicAdd(&lcnt[qme], 1u);
                if (p < (uint32_t)I8S_SL) lbuf[qme][p] = (uint32_t)row;
                else append_candidate(a, qme, row);  // this block's slots of the query are full
            }
        }
    };

    // every issue is unconditional (past the block's last step it repeats that step), so each wait
    // for a buffer counts the other buffer's loads and nothing else
    const int64_t s0 = t0 * SPT, s1 = t1 * SPT;
    Step A, B;
    issue(s0, A);
    for (int64_t s = s0; s < s1; s += 2) {
        issue(min(s + 1, s1 - 1), B);
        consume(s, A);
        issue(min(s + 2, s1 - 1), A);
        if (s + 1 < s1) consume(s + 1, B);
    }
    if constexpr (!DUMP) {
        __syncthreads();
        if (tid < NQ) {
            const uint32_t n = min(lcnt[tid], (uint32_t)I8S_SL);
            if (n) {
                const uint32_t base = atomicAdd(&a.cnt[tid], n);
                for (uint32_t i = 0; i < n; ++i)
                    if (base + i < (uint32_t)a.cap) a.cand[(int64_t)tid * a.cap + base + i] = lbuf[tid][i];
            }
        }
    }
}

// One dispatch of the streaming filter over local rows [c0, c1) (c0 a multiple of 128) for the
// nq <= 8 prepared query slots of ws (prepare_queries_i8_kernel); dump != null: the DUMP form.
// The grid is sized here, from the row count: i8s_bpc blocks per compute unit, each a run of tiles.
void launch_filter_i8_stream(const BatchPlan &p, const BatchWs &ws, int64_t c0, int64_t c1, float *dump, hipStream_t s) {
    RC_REQUIRE(p.nq >= 1 && p.nq <= I8_STREAM_MAX_QUERIES, RC_ERR_INVALID, "internal: the streaming int8 filter takes 1 to 8 queries");
    RC_REQUIRE(c0 % I8S_TILE == 0 && c0 < c1, RC_ERR_INVALID, "internal: streaming int8 filter range not tile-aligned");
    FilterI8StreamArgs fa{FilterArgs{p.rows8, ws.qh.get(), p.ld, 0, c0, c1, 0, 1, ws.thr.get(), ws.cnt.get(), ws.cand.get(), ws.cap}, dump, p.nq};
    fa.a.rsx = p.rsx;
    fa.a.rex = p.rex;
    fa.a.sq = ws.sq.get();
    fa.a.aq = ws.aq.get();
    const int64_t nt = (c1 - c0 + I8S_TILE - 1) / I8S_TILE;
    auto launch = [&](auto ld, auto nq) {
        constexpr int LD = decltype(ld)::value, NQ = decltype(nq)::value;
        fa.a.tiles_per_chunk = tiles_per_chunk(c0, c1, I8S_TILE, std::min<int64_t>(nt, I8S_CUS * i8s_bpc(LD, NQ)));
        const dim3 gr((unsigned)((nt + fa.a.tiles_per_chunk - 1) / fa.a.tiles_per_chunk)), bl(256);
        if (dump != nullptr) hipLaunchKernelGGL((filter_i8_stream_kernel<LD, NQ, true>), gr, bl, 0, s, fa);
        else hipLaunchKernelGGL((filter_i8_stream_kernel<LD, NQ, false>), gr, bl, 0, s, fa);
    };
    auto with_nq = [&](auto ld) {
        if (p.nq == 1) launch(ld, std::integral_constant<int, 1>{});
        else if (p.nq == 2) launch(ld, std::integral_constant<int, 2>{});
        else if (p.nq <= 4) launch(ld, std::integral_constant<int, 4>{});
        else launch(ld, std::integral_constant<int, 8>{});
    };
    if (p.ld == 256) with_nq(std::integral_constant<int, 256>{});
    else if (p.ld == 512) with_nq(std::integral_constant<int, 512>{});
    else if (p.ld == 768) with_nq(std::integral_constant<int, 768>{});
    else throw Error(RC_ERR_UNSUPPORTED, "int8 filter needs ld 256, 512 or 768");
    RC_LAUNCH_CHECK();
}

}  // namespace rc
