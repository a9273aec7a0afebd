// metafilter.hip — metadata columns on the device: rc_meta_write, rc_meta_move, rc_meta_eval.
//
// The columns of F indexed metadata fields over `capacity` rows are two arrays the caller owns
// (retrieval_core.h, "Metadata columns"): tags uint8 [F, capacity] and vals int64 [F, capacity],
// field-major, so the rows of one field are contiguous and a wave's 64 lanes read 64 B of tags
// and 512 B of vals per field, both coalesced.
//
// rc_meta_eval runs a postfix predicate program, one lane per position:
//   * the program is read through the constant address space (scalar loads: every lane runs the
//     same instruction, so the interpreter's control flow is wave-uniform and costs no VGPR);
//   * a lane's boolean stack is a 64-bit field in registers (bit 0 = top);
//   * a leaf loads its field's (tag, val) only when the field differs from the previous leaf's —
//     a wave-uniform branch; the compiler (metacolumns.compile_program) groups leaves by field;
//   * the wave ballots its answers, lane 0 stores the two uint32 words (plain vector stores), the
//     block adds its population count to the device counter with one atomic.
// The kernel is bound by the (1 + 8)-byte column reads; everything else is a few scalar and
// bit operations per instruction.
//
// Every argument, the program (field indices, stack discipline) and the page list are checked on
// the host before any device call; what the kernel then reads is the checked program (uploaded
// here, from the checked host copy) and column rows below `capacity`.
#include <vector>

#include "rc_common.h"

namespace rc {
namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void meta_write_kernel(uint8_t *__restrict__ tags, int64_t *__restrict__ vals, int F,
                                                            int64_t capacity, const int64_t *__restrict__ rows,
                                                            const uint8_t *__restrict__ in_tags,
                                                            const int64_t *__restrict__ in_vals, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int64_t r = rows[i];
    if (r < 0 || r >= capacity) return;  // never outside the columns, whatever the row list holds
    for (int f = 0; f < F; ++f) {
        tags[(int64_t)f * capacity + r] = in_tags[(int64_t)f * m + i];
        vals[(int64_t)f * capacity + r] = in_vals[(int64_t)f * m + i];
    }
}

__global__ __launch_bounds__(kBlock) void meta_move_kernel(uint8_t *__restrict__ tags, int64_t *__restrict__ vals, int F,
                                                           int64_t capacity, const int64_t *__restrict__ src,
                                                           const int64_t *__restrict__ dst, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int64_t s = src[i], d = dst[i];
    if (s < 0 || s >= capacity || d < 0 || d >= capacity) return;
    for (int f = 0; f < F; ++f) {
        tags[(int64_t)f * capacity + d] = tags[(int64_t)f * capacity + s];
        vals[(int64_t)f * capacity + d] = vals[(int64_t)f * capacity + s];
    }
}

typedef const __attribute__((address_space(4))) int64_t *const_i64;
typedef const __attribute__((address_space(4))) int32_t *const_i32;

// program: int64 [2 n_instr]: word 0 = op | field << 8 | operand tag << 16 | n << 32, word 1 = operand val.
__global__ __launch_bounds__(kBlock) void meta_eval_kernel(const uint8_t *__restrict__ tags, const int64_t *__restrict__ vals,
                                                           int64_t capacity, const int64_t *__restrict__ program, int n_instr,
                                                           const int32_t *__restrict__ pages, int span, int64_t n,
                                                           int64_t n_words, uint32_t *__restrict__ out_words,
                                                           uint32_t *__restrict__ out_count) {
    __shared__ uint32_t wave_count[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the wave's first position: 64-aligned, so the wave lies inside one page (span % 256 == 0)
    const int64_t p0 = (int64_t)blockIdx.x * kBlock + __builtin_amdgcn_readfirstlane(wave * 64);
    const int64_t p = p0 + lane;
    const bool live = p < n;
    int64_t row = p;
    if (pages != nullptr && p0 < n) {
        const int64_t e = p0 / span;
        row = (int64_t)((const_i32)pages)[e] * span + (p - e * span);
    }
    const const_i64 prog = (const_i64)program;
    uint64_t stack = 0;
    int cur = -1;  // the field whose (tag, val) the lane holds
    uint32_t t = 0;
    int64_t v = 0;
    for (int pc = 0; pc < n_instr; ++pc) {
        const int64_t w0 = prog[2 * pc], ov = prog[2 * pc + 1];
        const int op = (int)(w0 & 0xff);
        if (op <= RC_META_NOT_EXISTS) {
            const int f = (int)((w0 >> 8) & 0xff);
            if (f != cur) {
                cur = f;
                if (live) {
                    t = tags[(int64_t)f * capacity + row];
                    v = vals[(int64_t)f * capacity + row];
                }
            }
            const uint32_t ot = (uint32_t)((w0 >> 16) & 0xff);
            const double a = __longlong_as_double(v), b = __longlong_as_double(ov);
            const bool num = t == RC_META_TAG_NUMBER && ot == RC_META_TAG_NUMBER;
            const bool eq = t == ot && (t == RC_META_TAG_NUMBER ? a == b : v == ov);
            bool r;
            switch (op) {
            case RC_META_EQ: r = eq; break;
            case RC_META_NE: r = !eq; break;
            case RC_META_GT: r = num && a > b; break;
            case RC_META_GE: r = num && a >= b; break;
            case RC_META_LT: r = num && a < b; break;
            case RC_META_LE: r = num && a <= b; break;
            case RC_META_EXISTS: r = t != RC_META_TAG_ABSENT; break;
            default: r = t == RC_META_TAG_ABSENT; break;
            }
            stack = (stack << 1) | (r ? 1u : 0u);
        } else if (op == RC_META_TRUE || op == RC_META_FALSE) {
            stack = (stack << 1) | (op == RC_META_TRUE ? 1u : 0u);
        } else {  // AND(k) / OR(k) over the top k entries
            const int k = (int)(w0 >> 32);
            const uint64_t m = k >= 64 ? ~0ull : ((1ull << k) - 1);
            const uint64_t top = stack & m;
            const bool r = op == RC_META_AND ? top == m : top != 0;
            stack = (k >= 64 ? 0ull : (stack >> k) << 1) | (r ? 1u : 0u);
        }
    }
    const bool ok = live && (stack & 1);
    const uint64_t bal = __ballot(ok);
    if (lane == 0) {
        const int64_t w = p0 >> 5;
        if (w < n_words) out_words[w] = (uint32_t)bal;
        if (w + 1 < n_words) out_words[w + 1] = (uint32_t)(bal >> 32);
        wave_count[wave] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
#pragma unroll
        for (int i = 0; i < kBlock / 64; ++i) c += wave_count[i];
        if (c) atomicAdd(out_count, c);
    }
}

void check_columns(const void *tags, const void *vals, int n_fields, int64_t capacity) {
    RC_REQUIRE(tags && vals, RC_ERR_INVALID, "null column buffer");
    RC_REQUIRE(n_fields >= 1 && n_fields <= RC_META_MAX_FIELDS, RC_ERR_INVALID, "n_fields must be in [1, RC_META_MAX_FIELDS]");
    RC_REQUIRE(capacity >= 1, RC_ERR_INVALID, "capacity must be positive");
}

// The program is well formed: known ops, fields < n_fields, operand tags of a value, the stack
// never underflows or passes RC_META_MAX_STACK, and exactly one entry is left.
void check_program(const int64_t *program, int n_instr, int n_fields) {
    RC_REQUIRE(program, RC_ERR_INVALID, "null program");
    RC_REQUIRE(n_instr >= 1 && n_instr <= RC_META_MAX_INSTR, RC_ERR_INVALID, "program length must be in [1, RC_META_MAX_INSTR]");
    int depth = 0;
    for (int pc = 0; pc < n_instr; ++pc) {
        const int64_t w0 = program[2 * pc];
        const int op = (int)(w0 & 0xff), f = (int)((w0 >> 8) & 0xff), ot = (int)((w0 >> 16) & 0xff);
        const int64_t k = w0 >> 32;
        RC_REQUIRE(w0 >= 0 && ((w0 >> 24) & 0xff) == 0, RC_ERR_INVALID, "malformed program word");
        if (op <= RC_META_NOT_EXISTS) {
            RC_REQUIRE(f < n_fields, RC_ERR_INVALID, "program names a field at or past n_fields");
            if (op <= RC_META_LE)
                RC_REQUIRE(ot >= RC_META_TAG_NUMBER && ot <= RC_META_TAG_STRING, RC_ERR_INVALID, "bad operand tag");
            depth += 1;
        } else if (op == RC_META_TRUE || op == RC_META_FALSE) {
            depth += 1;
        } else if (op == RC_META_AND || op == RC_META_OR) {
            RC_REQUIRE(k >= 1 && k <= depth, RC_ERR_INVALID, "program underflows its stack");
            depth -= (int)k - 1;
        } else {
            RC_REQUIRE(false, RC_ERR_INVALID, "unknown program op");
        }
        RC_REQUIRE(depth <= RC_META_MAX_STACK, RC_ERR_INVALID, "program passes RC_META_MAX_STACK");
    }
    RC_REQUIRE(depth == 1, RC_ERR_INVALID, "program must leave exactly one result");
}

}  // namespace
}  // namespace rc

using namespace rc;

extern "C" {

int rc_meta_write(uint8_t *tags, int64_t *vals, int n_fields, int64_t capacity, const int64_t *rows, const uint8_t *in_tags,
                  const int64_t *in_vals, int64_t n, void *stream) {
    return guard([&] {
        check_columns(tags, vals, n_fields, capacity);
        RC_REQUIRE(n >= 0 && n <= capacity, RC_ERR_INVALID, "row count outside [0, capacity]");
        if (n == 0) return;
        RC_REQUIRE(rows && in_tags && in_vals, RC_ERR_INVALID, "null buffer");
        hipLaunchKernelGGL(meta_write_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                           tags, vals, n_fields, capacity, rows, in_tags, in_vals, n);
        RC_LAUNCH_CHECK();
    });
}

int rc_meta_move(uint8_t *tags, int64_t *vals, int n_fields, int64_t capacity, const int64_t *src_rows,
                 const int64_t *dst_rows, int64_t n, void *stream) {
    return guard([&] {
        check_columns(tags, vals, n_fields, capacity);
        RC_REQUIRE(n >= 0 && n <= capacity, RC_ERR_INVALID, "row count outside [0, capacity]");
        if (n == 0) return;
        RC_REQUIRE(src_rows && dst_rows, RC_ERR_INVALID, "null buffer");
        hipLaunchKernelGGL(meta_move_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                           tags, vals, n_fields, capacity, src_rows, dst_rows, n);
        RC_LAUNCH_CHECK();
    });
}

int rc_meta_eval(const uint8_t *tags, const int64_t *vals, int n_fields, int64_t capacity, const int64_t *program_host,
                 int n_instr, const int32_t *pages_host, int n_pages, int span, int64_t n, void *workspace,
                 int64_t workspace_bytes, uint32_t *out_words, uint32_t *out_count, void *stream) {
    return guard([&] {
        check_columns(tags, vals, n_fields, capacity);
        check_program(program_host, n_instr, n_fields);
        RC_REQUIRE(n >= 0 && n < ((int64_t)1 << 32), RC_ERR_INVALID, "n must be in [0, 2^32)");
        RC_REQUIRE(out_count, RC_ERR_INVALID, "null count buffer");
        RC_REQUIRE(n == 0 || out_words, RC_ERR_INVALID, "null bitmap buffer");
        RC_REQUIRE(n_pages >= 0, RC_ERR_INVALID, "negative page count");
        const bool paged = pages_host != nullptr;
        if (paged) {
            RC_REQUIRE(span >= 256 && span % 256 == 0, RC_ERR_INVALID, "span must be a positive multiple of 256");
            RC_REQUIRE(n <= (int64_t)n_pages * span, RC_ERR_INVALID, "n beyond the page list");
            const int64_t limit = capacity / span;  // whole pages inside the columns
            for (int i = 0; i < n_pages; ++i)
                RC_REQUIRE(pages_host[i] >= 0 && pages_host[i] < limit, RC_ERR_INVALID, "page at or past capacity / span");
        } else {
            RC_REQUIRE(n_pages == 0, RC_ERR_INVALID, "a page count without a page list");
            RC_REQUIRE(n <= capacity, RC_ERR_INVALID, "n beyond the capacity");
        }
        const size_t prog_bytes = (size_t)n_instr * 16, page_bytes = paged ? (size_t)n_pages * 4 : 0;
        RC_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, RC_ERR_INVALID, "the workspace must be 16-byte aligned");
        RC_REQUIRE(workspace_bytes >= 0 && (size_t)workspace_bytes >= prog_bytes + page_bytes, RC_ERR_INVALID,
                   "the workspace is smaller than 16 n_instr + 4 n_pages bytes");
        hipStream_t s = (hipStream_t)stream;
        RC_HIP(hipMemsetAsync(out_count, 0, sizeof(uint32_t), s));
        if (n == 0) return;
        int64_t *prog_dev = (int64_t *)workspace;
        int32_t *pages_dev = paged ? (int32_t *)((uint8_t *)workspace + prog_bytes) : nullptr;
        RC_HIP(hipMemcpyAsync(prog_dev, program_host, prog_bytes, hipMemcpyHostToDevice, s));
        if (page_bytes) RC_HIP(hipMemcpyAsync(pages_dev, pages_host, page_bytes, hipMemcpyHostToDevice, s));
        const int64_t n_words = (n + 31) / 32;
        hipLaunchKernelGGL(meta_eval_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, tags, vals, capacity,
                           prog_dev, n_instr, pages_dev, span, n, n_words, out_words, out_count);
        RC_LAUNCH_CHECK();
    });
}

}  // extern "C"
