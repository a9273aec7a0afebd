// inflate_check — the device inflate's host-checkable core (csrc/inflate_core.h: bit reader, table
// build, block header, single-token decode), run serially on the CPU against zlib.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I <pkg>/csrc tools/inflate_check.cpp -lz -o inflate_check
//   inflate_check FILE...
//
// A FILE is a PNG (its IDAT bodies are joined; CRCs are not looked at) or a bare zlib stream.  For
// each, the stream is inflated with exactly the functions the kernels use and with zlib; the two
// must agree on the verdict (a complete stream with a matching Adler-32, or not) and, when both
// accept, on every byte.  Exit status 1 at the first disagreement.  Built with the sanitizers, a
// run over the test corpus and its damaged variants is the memory-safety check of that code: the
// stream's bytes are in a heap block of their exact size.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "inflate_core.h"

using namespace rc::inflate;

static const size_t kLimit = (size_t)1 << 28;

static bool inflate_core(const std::vector<uint8_t> &z, std::vector<uint8_t> &out) {
    const size_t n = z.size();
    if (n < 6 || n > ((size_t)1 << 26)) return false;
    if ((z[0] & 15) != 8 || (z[0] >> 4) > 7 || ((z[0] << 8) | z[1]) % 31 || (z[1] & 32)) return false;
    std::vector<uint32_t> w((n + 3) / 4, 0u);
    std::memcpy(w.data(), z.data(), n);
    const Bits b = {w.data(), (int32_t)w.size()};
    const int32_t nbits = (int32_t)(n * 8);
    const Serial co;
    std::vector<uint8_t> lens(kLitSyms + kDistSyms + 8), cl(kClSyms);
    std::vector<Huff> tab(2);
    Huff &lit = tab[0], &dst = tab[1];
    int32_t p = 16;
    for (;;) {
        if (p + 3 > nbits) return false;
        const BlockHdr h = read_block_header(b, p, cl.data());
        if (h.bad || h.p > nbits) return false;
        p = h.p;
        if (h.btype == 0) {
            const size_t bp = ((size_t)p + 7) >> 3;
            if (bp + 4 > n) return false;
            const uint32_t len = z[bp] | z[bp + 1] << 8, nlen = z[bp + 2] | z[bp + 3] << 8;
            if (len != (~nlen & 0xFFFFu) || bp + 4 + len > n || out.size() + len > kLimit) return false;
            out.insert(out.end(), z.begin() + bp + 4, z.begin() + bp + 4 + len);
            p = (int32_t)((bp + 4 + len) * 8);
        } else {
            if (h.btype == 1) {
                fixed_lengths(lens.data(), co);
                huff_build(lit, lens.data(), kLitSyms, kLitLook, true, co);
                huff_build(dst, lens.data() + kLitSyms, kDistSyms, kDistLook, true, co);
            } else {
                huff_build(dst, cl.data(), kClSyms, kClLook, false, co);
                if (dst.bad) return false;
                int32_t bad = 0;
                p = read_code_lengths(dst, b, p, h.nlen + h.ndist, lens.data(), bad);
                if (bad || p > nbits || lens[256] == 0) return false;
                huff_build(lit, lens.data(), h.nlen, kLitLook, true, co);
                huff_build(dst, lens.data() + h.nlen, h.ndist, kDistLook, true, co);
                if (lit.bad || dst.bad) return false;
            }
            for (;;) {
                const Token t = decode_token(lit, dst, b, p);
                if (t.kind == TOK_INVALID || p + t.bits > nbits) return false;
                p += t.bits;
                if (t.kind == TOK_END) break;
                if (t.kind == TOK_LITERAL) {
                    out.push_back((uint8_t)t.val);
                } else {
                    if ((size_t)t.dist > out.size()) return false;
                    for (int k = 0; k < t.val; ++k) out.push_back(out[out.size() - (size_t)t.dist]);
                }
                if (out.size() > kLimit) return false;
            }
        }
        if (h.bfinal) break;
    }
    const size_t bp = ((size_t)p + 7) >> 3;
    if (bp + 4 > n) return false;
    uint32_t a = 1, s = 0;
    for (uint8_t c : out) {
        a = (a + c) % 65521u;
        s = (s + a) % 65521u;
    }
    const uint32_t want = (uint32_t)z[bp] << 24 | (uint32_t)z[bp + 1] << 16 | (uint32_t)z[bp + 2] << 8 | z[bp + 3];
    return want == ((s << 16) | a);
}

static bool inflate_zlib(const std::vector<uint8_t> &z, std::vector<uint8_t> &out) {
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (inflateInit(&zs) != Z_OK) return false;
    zs.next_in = const_cast<Bytef *>(z.data());
    zs.avail_in = (uInt)z.size();
    std::vector<uint8_t> buf(1 << 16);
    int r = Z_OK;
    while (r == Z_OK && out.size() <= kLimit) {
        zs.next_out = buf.data();
        zs.avail_out = (uInt)buf.size();
        r = inflate(&zs, Z_NO_FLUSH);
        out.insert(out.end(), buf.data(), buf.data() + (buf.size() - zs.avail_out));
        if (r == Z_OK && zs.avail_in == 0 && zs.avail_out != 0) break;  // the input ran out
    }
    inflateEnd(&zs);
    return r == Z_STREAM_END;
}

static std::vector<uint8_t> idat_of(const std::vector<uint8_t> &f) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    if (f.size() < 8 || std::memcmp(f.data(), sig, 8)) return f;  // a bare zlib stream
    std::vector<uint8_t> z;
    size_t at = 8;
    while (at + 12 <= f.size()) {
        const size_t len = (size_t)f[at] << 24 | (size_t)f[at + 1] << 16 | (size_t)f[at + 2] << 8 | f[at + 3];
        if (at + 12 + len > f.size()) break;
        if (!std::memcmp(f.data() + at + 4, "IDAT", 4)) z.insert(z.end(), f.begin() + at + 8, f.begin() + at + 8 + len);
        at += 12 + len;
    }
    return z;
}

int main(int argc, char **argv) {
    int bad = 0;
    for (int i = 1; i < argc; ++i) {
        FILE *fp = std::fopen(argv[i], "rb");
        if (!fp) {
            std::fprintf(stderr, "%s: cannot open\n", argv[i]);
            return 2;
        }
        std::vector<uint8_t> f;
        uint8_t chunk[1 << 16];
        for (size_t got; (got = std::fread(chunk, 1, sizeof(chunk), fp)) > 0;) f.insert(f.end(), chunk, chunk + got);
        std::fclose(fp);
        const std::vector<uint8_t> z = idat_of(f);
        std::vector<uint8_t> a, b;
        const bool ok_core = inflate_core(z, a), ok_zlib = inflate_zlib(z, b);
        const bool same = ok_core == ok_zlib && (!ok_core || a == b);
        std::printf("%s: %zu bytes, core %s, zlib %s, %zu inflated: %s\n", argv[i], z.size(), ok_core ? "accepts" : "refuses",
                    ok_zlib ? "accepts" : "refuses", b.size(), same ? "agree" : "DISAGREE");
        bad += !same;
    }
    return bad ? 1 : 0;
}
