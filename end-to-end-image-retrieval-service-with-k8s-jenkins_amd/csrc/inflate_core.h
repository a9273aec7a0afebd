// inflate_core.h — the parts of a DEFLATE decoder that the GPU kernels (png_inflate.hip) and the
// serial host check (tools/inflate_check.cpp) share word for word: the bit reader, the Huffman
// table build, the block header and the decode of one token.  Plain C++, no HIP type; on the
// device the same functions run with a workgroup cooperating on the table build.
//
// Bits.  The stream is held as little-endian dwords, so bit k of the stream is bit (k & 31) of
// dword k >> 5 and a field's least significant bit comes first, as DEFLATE packs it.  peek() is
// the only reader: it range-checks both dwords it touches and reads zeros outside.
//
// Tables (one Huff per alphabet): count[l] codes of length l, first[l] the canonical code of the
// first of them, offset[l] where they start in `sorted` (the symbols by length, then by value),
// and a lookahead table over the next `lookbits` bits (as they come, i.e. the code bit-reversed)
// that resolves every code of at most that length with one read.  Longer codes reverse 15 bits
// and walk the lengths lookbits+1..15.
//
// Token.  One literal, one end-of-block, or one whole match (length code, its extra bits, distance
// code, its extra bits: at most 15 + 5 + 15 + 13 = 48 bits).  A decoder's state inside a block is
// therefore a bit position and nothing else.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RC_HD __host__ __device__ __forceinline__
#else
#define RC_HD inline
#endif

namespace rc {
namespace inflate {

constexpr int kLitSyms = 288, kDistSyms = 32, kClSyms = 19;
constexpr int kLitLook = 10, kDistLook = 8, kClLook = 7;
constexpr int kMaxToken = 48;  // bits

struct Bits {
    const uint32_t *w;
    int32_t ndw;
};

// 32 bits of the stream from bit p on (zeros outside [0, 32 ndw)).
RC_HD uint32_t peek(const Bits &b, int32_t p) {
    const uint32_t i = (uint32_t)(p >> 5);
    const uint32_t lo = i < (uint32_t)b.ndw ? b.w[i] : 0u;
    const uint32_t hi = i + 1u < (uint32_t)b.ndw ? b.w[i + 1u] : 0u;
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (p & 31));
}

RC_HD uint32_t rev32(uint32_t v) {
#if defined(__clang__)
    return __builtin_bitreverse32(v);  // v_bfrev_b32 on the device
#else
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    return __builtin_bswap32(v);
#endif
}

struct Huff {
    uint16_t look[1 << kLitLook];  // symbol | length << 9; 0: no code of <= lookbits bits here
    uint16_t sorted[kLitSyms];
    uint32_t count[16];
    uint16_t first[16], offset[16];
    int32_t lookbits;
    int32_t bad;  // over-subscribed, or incomplete in a way zlib refuses
};

// The caller of huff_build: one thread (the host check) or a workgroup (the kernel).
struct Serial {
    RC_HD int id() const { return 0; }
    RC_HD int n() const { return 1; }
    RC_HD void sync() const {}
    RC_HD void inc(uint32_t *p) const { ++*p; }
};

// Build `h` from n code lengths (0: unused).  allow_one: a set whose only code is one of length 1
// is accepted though incomplete (zlib: literal/length and distance sets, not the code-length set);
// a set with no code at all is accepted too, and any decode from it fails.
template <class C>
RC_HD void huff_build(Huff &h, const uint8_t *lens, int n, int lookbits, bool allow_one, const C &co) {
    for (int i = co.id(); i < (1 << kLitLook); i += co.n()) h.look[i] = 0;
    for (int i = co.id(); i < 16; i += co.n()) h.count[i] = 0;
    co.sync();
    for (int s = co.id(); s < n; s += co.n()) {
        const int l = lens[s] & 15;
        if (l) co.inc(&h.count[l]);
    }
    co.sync();
    if (co.id() == 0) {
        int code = 0, off = 0, left = 1, maxl = 0, bad = 0;
        h.first[0] = h.offset[0] = 0;
        for (int l = 1; l <= 15; ++l) {
            const int c = (int)h.count[l];
            left = (left << 1) - c;
            if (left < 0) {
                bad = 1;  // over-subscribed
                left = 0;
            }
            code <<= 1;
            h.first[l] = (uint16_t)code;
            h.offset[l] = (uint16_t)off;
            code += c;
            off += c;
            if (c) maxl = l;
        }
        if (left > 0 && maxl != 0 && !(allow_one && maxl == 1)) bad = 1;  // incomplete
        h.bad = bad;
        h.lookbits = lookbits;
    }
    co.sync();
    const bool bad = h.bad != 0;
    for (int s = co.id(); s < n; s += co.n()) {
        const int l = lens[s] & 15;
        if (!l || bad) continue;
        int rank = 0;  // symbols of the same length before this one
        for (int j = 0; j < s; ++j) rank += (lens[j] & 15) == l;
        const int idx = h.offset[l] + rank;
        if (idx < kLitSyms) h.sorted[idx] = (uint16_t)s;
        if (l <= lookbits) {
            const uint32_t code = ((uint32_t)h.first[l] + (uint32_t)rank) & ((1u << l) - 1u);
            const uint32_t rev = rev32(code) >> (32 - l);
            for (uint32_t k = rev; k < (1u << lookbits); k += 1u << l) h.look[k] = (uint16_t)(s | (l << 9));
        }
    }
    co.sync();
}

// The symbol whose code starts at bit 0 of v, and its length; -1: no code of the set.
RC_HD int decode_sym(const Huff &h, uint32_t v, int &len) {
    const int lb = h.lookbits & 15;
    const uint32_t e = h.look[v & ((1u << lb) - 1u) & ((1u << kLitLook) - 1u)];
    if (e) {
        len = (int)(e >> 9);
        return (int)(e & 511u);
    }
    const uint32_t rev = rev32(v) >> 17;  // 15 bits, first bit on top: canonical order
    for (int l = lb + 1; l <= 15; ++l) {
        const uint32_t idx = (rev >> (15 - l)) - (uint32_t)h.first[l];
        if (idx < h.count[l]) {
            const uint32_t j = (uint32_t)h.offset[l] + idx;
            if (j >= (uint32_t)kLitSyms) return -1;
            len = l;
            return (int)h.sorted[j];
        }
    }
    return -1;
}

enum : int32_t { TOK_LITERAL = 0, TOK_MATCH = 1, TOK_END = 2, TOK_INVALID = 3 };

struct Token {
    int32_t kind, bits;  // an invalid token takes one bit: a decoder in a wrong state moves on
    int32_t val, dist;   // the literal, or the match's length and distance
};

RC_HD Token decode_token(const Huff &lit, const Huff &dst, const Bits &b, int32_t p) {
    Token t = {TOK_INVALID, 1, 0, 0};
    uint32_t v = peek(b, p);
    int len = 1;
    const int s = decode_sym(lit, v, len);
    if (s < 0 || s > 285) return t;
    if (s < 256) return Token{TOK_LITERAL, len, s, 0};
    if (s == 256) return Token{TOK_END, len, 0, 0};
    int n = len, length;
    if (s < 265) {
        length = s - 254;
    } else if (s == 285) {
        length = 258;
    } else {
        const int i = s - 257, e = (i >> 2) - 1;
        length = 3 + ((4 + (i & 3)) << e) + (int)((v >> n) & ((1u << e) - 1u));
        n += e;
    }
    v = peek(b, p + n);
    int dl = 1;
    const int ds = decode_sym(dst, v, dl);
    if (ds < 0 || ds > 29) return t;
    int dist;
    if (ds < 4) {
        dist = ds + 1;
    } else {
        const int e = (ds >> 1) - 1;
        dist = 1 + ((2 + (ds & 1)) << e) + (int)((v >> dl) & ((1u << e) - 1u));
        dl += e;
    }
    return Token{TOK_MATCH, n + dl, length, dist};
}

// ------------------------------------------------------------------ block header --
struct BlockHdr {
    int32_t bfinal, btype;
    int32_t nlen, ndist;  // dynamic: literal/length and distance code lengths that follow
    int32_t p;            // the bit after what was read
    int32_t bad;
};

// BFINAL, BTYPE and, of a dynamic block, HLIT / HDIST / HCLEN and the code-length set's lengths
// (cl: kClSyms entries).
RC_HD BlockHdr read_block_header(const Bits &b, int32_t p, uint8_t *cl) {
    const uint8_t order[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    BlockHdr h = {0, 0, 0, 0, 0, 0};
    uint32_t v = peek(b, p);
    h.bfinal = (int32_t)(v & 1u);
    h.btype = (int32_t)((v >> 1) & 3u);
    p += 3;
    if (h.btype == 3) h.bad = 1;
    if (h.btype == 2) {
        v = peek(b, p);
        h.nlen = (int32_t)(v & 31u) + 257;
        h.ndist = (int32_t)((v >> 5) & 31u) + 1;
        const int ncl = (int)((v >> 10) & 15u) + 4;
        p += 14;
        if (h.nlen > 286 || h.ndist > 30) h.bad = 1;
        for (int i = 0; i < kClSyms; ++i) cl[order[i]] = 0;
        for (int i = 0; i < ncl; ++i) {
            cl[order[i]] = (uint8_t)(peek(b, p) & 7u);
            p += 3;
        }
    }
    h.p = p;
    return h;
}

// The `total` code lengths of a dynamic block, run-length coded with the set `cl`.  Returns the
// bit after them; bad: a code outside the set, a repeat with nothing before it or past the end.
RC_HD int32_t read_code_lengths(const Huff &cl, const Bits &b, int32_t p, int total, uint8_t *lens, int32_t &bad) {
    int i = 0;
    while (i < total) {  // every round stores at least one length or ends
        const uint32_t v = peek(b, p);
        int len = 1;
        const int s = decode_sym(cl, v, len);
        if (s < 0 || s > 18) {
            bad = 1;
            break;
        }
        p += len;
        if (s < 16) {
            lens[i++] = (uint8_t)s;
            continue;
        }
        int prev = 0, rep;
        if (s == 16) {
            if (i == 0) {
                bad = 1;
                break;
            }
            prev = lens[i - 1];
            rep = 3 + (int)((v >> len) & 3u);
            p += 2;
        } else if (s == 17) {
            rep = 3 + (int)((v >> len) & 7u);
            p += 3;
        } else {
            rep = 11 + (int)((v >> len) & 127u);
            p += 7;
        }
        if (i + rep > total) {
            bad = 1;
            break;
        }
        for (int k = 0; k < rep; ++k) lens[i++] = (uint8_t)prev;
    }
    return p;
}

// The fixed block's code lengths: lens[0..288) literal/length, lens[288..320) distance.
template <class C>
RC_HD void fixed_lengths(uint8_t *lens, const C &co) {
    for (int s = co.id(); s < kLitSyms + kDistSyms; s += co.n())
        lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    co.sync();
}

}  // namespace inflate
}  // namespace rc
