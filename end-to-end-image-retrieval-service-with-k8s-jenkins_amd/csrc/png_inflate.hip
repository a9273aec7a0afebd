// png_inflate.hip — DEFLATE on gfx950 for PNG image data: one workgroup of LANES lanes inflates
// one image's zlib stream into the library's device scanline buffer, token-parallel, and
// rc_png_decode runs png_reconstruct_kernel on what it produced.  DESIGN.md "PNG inflate on the
// device".  The decoder core (bit reader, table build, block header, single-token decode) is
// inflate_core.h, which tools/inflate_check.cpp runs serially on the host against zlib.
//
// The workgroup walks the stream in steps; a step is one block header or one window of tokens.
//   header   LANES + 8 dwords from the current bit on are copied to LDS.  Lane 0 reads BFINAL,
//            BTYPE and, of a dynamic block, the counts, the code-length set and (with that set's
//            table, built by all lanes) the run-length coded code lengths; all lanes then build
//            the literal/length and distance tables: per length a count (LDS atomics), first code
//            and offset, every symbol's rank among its length and from it the sorted symbol array
//            and the lookahead entries (10 bits literal/length, 8 distance).  A fixed block builds
//            the same tables from the constant lengths; a stored block is copied by all lanes.
//   window   LANES rows of ROW_BITS bits of the block.  The window is kept flat in LDS, so a row's
//            overhang (a token that starts in the row ends at most 47 bits past it) is the next
//            row's first bits and only the last row needs dwords of its own.  Synchronisation:
//            every lane decodes the tokens that start in its row from a guessed entry (the row's
//            first bit), publishes its exit (the bit after its last token), takes its left
//            neighbour's exit as entry and decodes again until no exit changes; a lane whose entry
//            did not change does not decode.  Lane 0's entry is true, so after round j lanes
//            0..j-1 are: at most LANES + 1 rounds.  A lane that meets end-of-block marks its exit;
//            the lanes to its right go dead.  Output positions: a block scan of the bytes and of
//            the matches per lane.  Write: the lanes decode once more from their true entries,
//            store literals and queue matches (destination, distance, length) in stream order,
//            QUEUE at a time; the queue is resolved in rounds: with F the first queued match's
//            destination, all bytes below F are final, and the run of following matches whose
//            source ends at or below F is copied at once, 16 lanes to a match; the head match may
//            overlap its own output (distance < length) and is written by period replication,
//            byte k from source byte k mod distance.  The history is the scanline buffer itself.
//   end      final block seen, exactly scan_bytes produced, the Adler-32 behind the last block
//            (computed here from per-lane sums, combined mod 65521) and every filter byte <= 4;
//            anything else raises the image's flag and the host inflates it.
//
// Memory safety.  The stream's bits select values only.  Every read of the stream goes through
// peek() on the LDS window (both dwords range-checked) or tests its dword index against the
// descriptor's ndw first; every table index is masked or compared with the table's size; every
// store tests its offset against scan_bytes; a match is queued only with distance <= bytes
// produced and destination + length <= scan_bytes, else the flag is raised and it is dropped.
// Loop bounds: the step count comes from the stream's length (a header takes >= 3 bits, a window
// without end-of-block >= LANES * ROW_BITS); sync rounds <= LANES + 1; a row holds <= ROW_BITS
// tokens; queue batches <= window bits / QUEUE + 1; resolve rounds <= QUEUE.
#include <vector>

#include "inflate_core.h"
#include "png_host.h"

namespace rc {
namespace pngz {

using namespace rc::inflate;

constexpr int LANES = RC_PNG_INFLATE_LANES;
constexpr int ROW_BITS = RC_PNG_INFLATE_ROW_BITS;
constexpr int WIN_BITS = LANES * ROW_BITS;
constexpr int WIN_DW = WIN_BITS / 32 + 8;  // the window, the bit offset of its start, the last row's overhang
constexpr int QUEUE = 1024;                // matches resolved per batch
constexpr int NWAVE = LANES / 64;
constexpr uint32_t EX_END = 0x80000000u;   // exit: end-of-block met, the bit after it below
constexpr uint32_t EX_DEAD = 0xFFFFFFFFu;  // exit of a lane right of the end-of-block
static_assert(ROW_BITS >= 2 * kMaxToken && ROW_BITS % 32 == 0, "a token spans at most two rows");
static_assert(WIN_BITS + 32 + kMaxToken + 64 <= WIN_DW * 32, "the last row's reads stay inside the window");

struct IDesc {
    int64_t in_off;    // the zlib stream in the upload, bytes (a multiple of 4)
    int64_t scan_off;  // the image's scanlines in the scanline buffer (a multiple of 256)
    int32_t nbytes;    // bytes of the stream
    int32_t ndw;       // dwords of it in the upload (the last one zero-padded)
    int32_t scan_bytes;  // height * (1 + stride): what it must inflate to
    int32_t pitch;     // 1 + stride
    int32_t height, pad;
};

struct Block {  // the workgroup as huff_build's caller
    __device__ __forceinline__ int id() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int n() const { return LANES; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ void inc(uint32_t *p) const { atomicAdd(p, 1u); }
};

struct Shared {
    uint32_t win[WIN_DW];
    Huff lit, dst;  // dst also holds the code-length set's table while a dynamic header is read
    uint8_t lens[kLitSyms + kDistSyms + 8];
    uint8_t cl[kClSyms + 1];
    uint32_t ex[LANES];
    uint32_t qdst[QUEUE], qmd[QUEUE];  // a match's destination; distance | length << 16 (0: dropped)
    uint32_t wsum[2][NWAVE];
    uint32_t wfail[NWAVE];
    BlockHdr hdr;
    int32_t bad, endlane;
    uint32_t stored_len;
};

// Exclusive block scan of two counters; the totals in ta / tb.  Two barriers.
__device__ __forceinline__ void scan2(Shared &S, uint32_t a, uint32_t b, uint32_t &xa, uint32_t &xb, uint32_t &ta,
                                      uint32_t &tb) {
    const int wl = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t ia = a, ib = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ya = __shfl_up(ia, d), yb = __shfl_up(ib, d);
        if (wl >= d) ia += ya, ib += yb;
    }
    __syncthreads();
    if (wl == 63) S.wsum[0][wv] = ia, S.wsum[1][wv] = ib;
    __syncthreads();
    ta = tb = 0;
#pragma unroll
    for (int j = 0; j < NWAVE; ++j) {
        if (j < wv) ia += S.wsum[0][j], ib += S.wsum[1][j];
        ta += S.wsum[0][j], tb += S.wsum[1][j];
    }
    xa = ia - a, xb = ib - b;
}

// The tokens that start in [entry, lim): nothing stored, an invalid code takes one bit.
__device__ __forceinline__ uint32_t sync_row(const Shared &S, const Bits &b, uint32_t entry, int lim, uint32_t &nby,
                                             uint32_t &nm) {
    int p = (int)entry;
    nby = nm = 0;
    for (int it = 0; it < ROW_BITS && p < lim; ++it) {
        const Token t = decode_token(S.lit, S.dst, b, p);
        p += t.bits;
        if (t.kind == TOK_LITERAL) nby += 1;
        if (t.kind == TOK_MATCH) nby += (uint32_t)t.val, nm += 1;
        if (t.kind == TOK_END) return EX_END | (uint32_t)p;
    }
    return (uint32_t)p;
}

// Resolve the first cnt queued matches (stream order).  Uniform control flow.
__device__ __forceinline__ void resolve(Shared &S, uint8_t *out, int cnt) {
    const int tid = (int)threadIdx.x, wl = tid & 63, wv = tid >> 6;
    int head = 0;
    for (int round = 0; round < QUEUE && head < cnt; ++round) {  // every round takes the head match at least
        const uint32_t F = S.qdst[head];
        const int i = head + tid;
        bool ready = false;
        if (i < cnt) {
            const uint32_t md = S.qmd[i], dist = md & 0xFFFFu, len = md >> 16;
            ready = i == head || md == 0u || S.qdst[i] - dist + min(len, dist) <= F;
        }
        const unsigned long long m = __ballot(ready);
        if (wl == 0) S.wfail[wv] = m == ~0ull ? 64u : (uint32_t)__ffsll((long long)~m) - 1u;
        __syncthreads();
        int run = 0;
#pragma unroll
        for (int j = 0; j < NWAVE; ++j) {
            if (run == 64 * j) run += (int)S.wfail[j];
        }
        run = max(1, min(run, cnt - head));
        for (int k = tid >> 4; k < run; k += LANES / 16) {
            const uint32_t md = S.qmd[head + k], dist = md & 0xFFFFu, len = md >> 16, d0 = S.qdst[head + k];
            if (md == 0u) continue;
            for (uint32_t j = tid & 15; j < len; j += 16) out[d0 + j] = out[d0 - dist + (j < dist ? j : j % dist)];
        }
        __syncthreads();  // the copies are visible to the workgroup before anything reads them
        head += run;
    }
}

__global__ __launch_bounds__(LANES) void png_inflate_kernel(const uint32_t *__restrict__ upload,
                                                           const IDesc *__restrict__ descs, uint8_t *scan,
                                                           int32_t *__restrict__ flags) {
    __shared__ Shared S;
    const IDesc d = descs[blockIdx.x];
    const int tid = (int)threadIdx.x;
    const uint32_t *src = upload + (d.in_off >> 2);
    uint8_t *out = scan + d.scan_off;
    const int nbits = d.nbytes * 8;  // nbytes <= 2^26 (the host checked)
    const uint32_t scan_bytes = (uint32_t)d.scan_bytes;
    const Block co;
    if (tid == 0) S.bad = 0;
    int bitpos = 16;    // behind the zlib header, which the host checked
    uint32_t opos = 0;  // bytes produced
    bool in_block = false, final_block = false, finished = false;
    const int max_steps = nbits / 3 + nbits / WIN_BITS + 4;
    __syncthreads();

    for (int step = 0; step < max_steps; ++step) {  // all conditions below are workgroup-uniform
        if (S.bad || bitpos >= nbits) break;
        const int dw0 = bitpos >> 5, off = bitpos & 31;
        __syncthreads();  // the last step's readers of the window are done
        for (int i = tid; i < WIN_DW; i += LANES) S.win[i] = dw0 + i < d.ndw ? src[dw0 + i] : 0u;
        __syncthreads();
        const Bits b = {S.win, WIN_DW};
        const int lim_all = nbits - dw0 * 32;  // the stream's end, in window bits

        if (!in_block) {
            // ------------------------------------------------------------ block header
            if (tid == 0) {
                S.hdr = read_block_header(b, off, S.cl);
                if (S.hdr.p > lim_all) S.hdr.bad = 1;
            }
            __syncthreads();
            const BlockHdr h = S.hdr;
            if (h.bad) break;
            final_block = h.bfinal != 0;
            int p = h.p;
            if (h.btype == 0) {
                const int bp = (dw0 * 32 + p + 7) >> 3;  // byte of LEN in the stream
                if (bp + 4 > d.nbytes) {
                    if (tid == 0) S.bad = 1;
                    break;
                }
                if (tid == 0) {  // LEN, NLEN: four bytes at any alignment; their dwords exist (bp + 4 <= nbytes)
                    const int q = bp * 8 - dw0 * 32;
                    const uint32_t v = q + 32 <= WIN_DW * 32 - 32 ? peek(b, q) : 0u;  // a header ends far inside the window
                    const uint32_t len = v & 0xFFFFu;
                    S.stored_len = len;
                    if ((v >> 16) != (~len & 0xFFFFu)) S.bad = 1;
                }
                __syncthreads();
                const uint32_t len = S.stored_len;
                const int data = bp + 4;
                if (S.bad || (int64_t)data + len > d.nbytes || opos + len > scan_bytes) {
                    if (tid == 0) S.bad = 1;
                    break;
                }
                const uint8_t *sb = reinterpret_cast<const uint8_t *>(src);  // data + len <= nbytes <= 4 ndw
                for (uint32_t i = tid; i < len; i += LANES) out[opos + i] = sb[data + i];
                opos += len;
                bitpos = (data + (int)len) * 8;
                if (final_block) {
                    finished = true;
                    break;
                }
                continue;
            }
            if (h.btype == 1) {
                fixed_lengths(S.lens, co);
                huff_build(S.lit, S.lens, kLitSyms, kLitLook, true, co);
                huff_build(S.dst, S.lens + kLitSyms, kDistSyms, kDistLook, true, co);
            } else {
                huff_build(S.dst, S.cl, kClSyms, kClLook, false, co);
                if (tid == 0) {
                    int32_t bad = S.dst.bad;
                    if (!bad) {
                        S.hdr.p = read_code_lengths(S.dst, b, p, h.nlen + h.ndist, S.lens, bad);
                        if (S.hdr.p > lim_all || S.lens[256] == 0) bad = 1;
                    }
                    S.hdr.bad = bad;
                }
                __syncthreads();
                if (S.hdr.bad) {
                    if (tid == 0) S.bad = 1;
                    break;
                }
                p = S.hdr.p;
                __syncthreads();
                huff_build(S.lit, S.lens, h.nlen, kLitLook, true, co);
                huff_build(S.dst, S.lens + h.nlen, h.ndist, kDistLook, true, co);
                if (S.lit.bad || S.dst.bad) {
                    if (tid == 0) S.bad = 1;
                    break;
                }
            }
            bitpos = dw0 * 32 + p;
            in_block = true;
            continue;
        }

        // ---------------------------------------------------------------- window of tokens
        const int row0 = off + tid * ROW_BITS;
        const int lim = min(row0 + ROW_BITS, lim_all);
        S.ex[tid] = (uint32_t)(row0 + ROW_BITS);  // the guess: the next row starts on a token
        if (tid == 0) S.endlane = LANES;
        __syncthreads();
        uint32_t used = EX_DEAD - 1u, exitv = 0, nby = 0, nm = 0, entry = 0;
        for (int it = 0; it <= LANES; ++it) {
            entry = tid == 0 ? (uint32_t)off : S.ex[tid - 1];
            __syncthreads();
            int changed = 0;
            if (entry != used) {
                used = entry;
                if (entry & EX_END) {
                    exitv = EX_DEAD;
                    nby = nm = 0;
                } else {
                    exitv = sync_row(S, b, entry, lim, nby, nm);
                }
                changed = exitv != S.ex[tid];
                S.ex[tid] = exitv;
            }
            if (!__syncthreads_or(changed)) break;
        }
        if ((exitv & EX_END) && exitv != EX_DEAD) atomicMin(&S.endlane, tid);
        uint32_t xby, xm, tby, tm;
        scan2(S, nby, nm, xby, xm, tby, tm);  // its barriers also publish endlane
        if (opos + tby > scan_bytes) {        // more than the image holds
            if (tid == 0) S.bad = 1;
            break;
        }
        // write: literals at once, matches through the queue
        int p = (int)entry;
        uint32_t op = opos + xby, mi = xm;
        bool done = (entry & EX_END) != 0;
        const int batches = max(1, (int)((tm + QUEUE - 1) / QUEUE));
        for (int bt = 0; bt < batches; ++bt) {  // tm <= WIN_BITS / 2
            const uint32_t lo = (uint32_t)bt * QUEUE;
            for (int it = 0; it < ROW_BITS && !done && p < lim; ++it) {
                const Token t = decode_token(S.lit, S.dst, b, p);
                if (t.kind == TOK_INVALID || p + t.bits > lim_all) {
                    S.bad = 1;
                    done = true;
                    break;
                }
                if (t.kind == TOK_MATCH) {
                    const uint32_t slot = mi - lo;
                    if (slot >= (uint32_t)QUEUE) break;  // the next batch's
                    const bool ok = (uint32_t)t.dist <= op && op + (uint32_t)t.val <= scan_bytes;
                    if (!ok) S.bad = 1;
                    S.qdst[slot] = op;
                    S.qmd[slot] = ok ? (uint32_t)t.dist | ((uint32_t)t.val << 16) : 0u;
                    op += (uint32_t)t.val;
                    ++mi;
                } else if (t.kind == TOK_LITERAL) {
                    if (op < scan_bytes) out[op] = (uint8_t)t.val;
                    ++op;
                } else {
                    done = true;
                }
                p += t.bits;
            }
            __syncthreads();  // queue and literals written
            resolve(S, out, (int)min((uint32_t)QUEUE, tm - min(tm, lo)));
            __syncthreads();
        }
        opos += tby;
        const int endlane = S.endlane;
        if (endlane < LANES) {
            bitpos = dw0 * 32 + (int)(S.ex[endlane] & ~EX_END);
            in_block = false;
            if (final_block) {
                finished = true;
                break;
            }
        } else {
            bitpos = dw0 * 32 + (int)S.ex[LANES - 1];
        }
    }

    // ------------------------------------------------------------------------ end of stream
    __syncthreads();
    bool good = finished && !S.bad && opos == scan_bytes;
    const int ab = (bitpos + 7) >> 3;  // the Adler-32, big-endian, on the byte behind the last block
    good = good && bitpos <= nbits && ab + 4 <= d.nbytes;
    if (!good) {  // uniform
        if (tid == 0) flags[blockIdx.x] = 1;
        return;
    }
    // a = 1 + sum d_i, b = N + sum (N - i) d_i  (mod 65521), a dword of four bytes at a time
    const uint32_t N = scan_bytes;
    const uint32_t *ow = reinterpret_cast<const uint32_t *>(out);  // the slice is 256-byte aligned and padded
    uint64_t sa = 0, sb = 0;
    for (uint32_t i = tid; i < (N + 3) / 4; i += LANES) {  // <= 2^17 dwords a lane: the sums stay below 2^54
        uint32_t v = ow[i];
        const uint32_t left = N - 4 * i;
        if (left < 4) v &= (1u << (8 * left)) - 1u;
        const uint32_t d0 = v & 255u, d1 = (v >> 8) & 255u, d2 = (v >> 16) & 255u, d3 = v >> 24;
        const uint32_t s = d0 + d1 + d2 + d3;
        sa += s;
        sb += (uint64_t)left * s - (d1 + 2 * d2 + 3 * d3);
    }
    uint32_t ra = (uint32_t)(sa % 65521u), rb = (uint32_t)(sb % 65521u), worst = 0;
    for (int r = tid; r < d.height; r += LANES) worst = max(worst, (uint32_t)out[(uint32_t)r * (uint32_t)d.pitch]);
    uint32_t xa, xb, ta, tb;
    scan2(S, ra, rb, xa, xb, ta, tb);  // the totals: at most LANES * 65520
    const uint32_t adler = (((N + tb) % 65521u) << 16) | ((1u + ta) % 65521u);
    uint32_t want = 0;
    for (int k = 0; k < 4; ++k) {
        const int q = ab + k;  // q < nbytes <= 4 ndw
        want = (want << 8) | ((src[q >> 2] >> (8 * (q & 3))) & 255u);
    }
    const int fail = __syncthreads_or(worst > 4u);
    if (tid == 0) flags[blockIdx.x] = (fail || adler != want) ? 1 : 0;
}

// ------------------------------------------------------------------------------- host --
// Per-device staging, grown geometrically and reused, with rc_png_reconstruct's rules: `staged`
// (the last upload has left the pinned block) is waited for before refilling, `done` (the last
// kernels) by the stream before it overwrites the device copies.
struct Workspace {
    std::mutex mu;
    PinBuf<uint8_t> h_stage;
    DevBuf<uint8_t> d_stage, d_scan;
    PinBuf<int32_t> h_flags;  // pinned read-back, kMaxImages entries
    hipEvent_t staged = nullptr, done = nullptr;
    int64_t device_images = 0, host_fallbacks = 0;
    // rc_png_decode_timing: an event pair around png_inflate_kernel alone, read after the call's
    // stream synchronise
    bool timing = false;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    double kernel_ms = 0.0;
    int64_t kernel_launches = 0;
};
constexpr int kMaxImages = 65535;

static Workspace &workspace(int device) {
    static Workspace *const ws = new Workspace[64];  // never destroyed: no device call runs at process exit
    RC_REQUIRE(device >= 0 && device < 64, RC_ERR_INVALID, "device ordinal out of range");
    return ws[device];
}

}  // namespace pngz
}  // namespace rc

using namespace rc;

extern "C" int rc_png_decode(int device, int n, const rc_png_stream *streams, uint8_t *rgb, int64_t rgb_bytes,
                             int32_t *flags_out, void *stream) {
    return guard([&] {
        RC_REQUIRE(n >= 1 && n <= pngz::kMaxImages, RC_ERR_INVALID, "image count must be 1..65535");
        RC_REQUIRE(streams && rgb && flags_out && rgb_bytes > 0, RC_ERR_INVALID, "null argument");
        auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
        // upload: inflate descriptors | reconstruction descriptors | flags | palettes | streams
        int npal = 0;
        for (int i = 0; i < n; ++i) npal += streams[i].color == 3;
        const size_t o_rdesc = al((size_t)n * sizeof(pngz::IDesc));
        const size_t o_flags = o_rdesc + al((size_t)n * sizeof(png::Desc));
        const size_t o_pal = o_flags + al((size_t)n * 4);
        const size_t o_data = o_pal + (size_t)npal * 1024;
        size_t total = o_data, scan_total = 0;
        std::vector<int64_t> strides(n);
        for (int i = 0; i < n; ++i) {
            const rc_png_stream &p = streams[i];
            const std::string id = "image " + std::to_string(i) + ": ";
            strides[i] = png::check_header(p, id);
            RC_REQUIRE(p.idat && p.idat_bytes >= 6, RC_ERR_INVALID, id + "no zlib stream of at least 6 bytes");
            RC_REQUIRE(p.idat_bytes <= RC_PNG_INFLATE_MAX_BYTES, RC_ERR_UNSUPPORTED,
                       id + "zlib stream above RC_PNG_INFLATE_MAX_BYTES");
            const unsigned cmf = p.idat[0], flg = p.idat[1];
            RC_REQUIRE((cmf & 15) == 8 && (cmf >> 4) <= 7 && ((cmf << 8) | flg) % 31 == 0 && !(flg & 32), RC_ERR_INVALID,
                       id + "zlib header is not deflate / 32 KiB window / no dictionary");
            png::check_palette_and_output(p, id, rgb_bytes);
            total += al((size_t)p.idat_bytes + 4);
            scan_total += al((size_t)p.height * (size_t)(1 + strides[i]));
        }
        RC_REQUIRE(total <= png::kMaxStageBytes && scan_total <= png::kMaxStageBytes, RC_ERR_UNSUPPORTED,
                   "the streams or scanlines of one call exceed the 512 MiB staging cap: split the batch");

        pngz::Workspace &ws = pngz::workspace(device);
        std::lock_guard<std::mutex> lock(ws.mu);
        DeviceScope ds(device);
        if (!ws.staged) RC_HIP(hipEventCreateWithFlags(&ws.staged, hipEventDisableTiming));
        if (!ws.done) RC_HIP(hipEventCreateWithFlags(&ws.done, hipEventDisableTiming));
        ws.h_flags.reserve((size_t)pngz::kMaxImages);
        RC_HIP(hipEventSynchronize(ws.staged));  // the last upload has left the pinned block
        if (const size_t cap = min_capacity(ws.h_stage, ws.d_stage); total > cap) {
            const size_t want = std::min(std::max(total, cap * 2), png::kMaxStageBytes);
            RC_HIP(hipDeviceSynchronize());  // a kernel may still read the old device copy
            ws.h_stage.reserve(want);
            ws.d_stage.reserve(want);
        }
        if (scan_total > ws.d_scan.capacity()) {
            RC_HIP(hipDeviceSynchronize());
            ws.d_scan.reserve(std::min(std::max(scan_total, ws.d_scan.capacity() * 2), png::kMaxStageBytes));
        }
        auto *idesc = reinterpret_cast<pngz::IDesc *>(ws.h_stage.get());
        auto *rdesc = reinterpret_cast<png::Desc *>(ws.h_stage.get() + o_rdesc);
        auto *pal = reinterpret_cast<uint32_t *>(ws.h_stage.get() + o_pal);
        std::memset(ws.h_stage.get() + o_flags, 0, (size_t)n * 4);
        size_t at = o_data, sat = 0;
        int ipal = 0;
        for (int i = 0; i < n; ++i) {
            const rc_png_stream &p = streams[i];
            pngz::IDesc &d = idesc[i];
            const size_t nb = (size_t)p.idat_bytes;
            d.in_off = (int64_t)at;
            d.scan_off = (int64_t)sat;
            d.nbytes = (int32_t)nb;
            d.ndw = (int32_t)((nb + 3) / 4);
            d.pitch = (int32_t)(1 + strides[i]);
            d.height = p.height;
            d.scan_bytes = (int32_t)((int64_t)p.height * d.pitch);  // <= 2^24 * 4 + 2^24
            d.pad = 0;
            png::fill_desc(rdesc[i], p, (int64_t)sat, pal, ipal);
            std::memcpy(ws.h_stage.get() + at, p.idat, nb);
            std::memset(ws.h_stage.get() + at + nb, 0, al(nb + 4) - nb);
            at += al(nb + 4);
            sat += al((size_t)d.scan_bytes);
        }
        hipStream_t s = (hipStream_t)stream;
        RC_HIP(hipStreamWaitEvent(s, ws.done, 0));
        RC_HIP(hipMemcpyAsync(ws.d_stage.get(), ws.h_stage.get(), total, hipMemcpyHostToDevice, s));
        RC_HIP(hipEventRecord(ws.staged, s));
        int32_t *d_flags = reinterpret_cast<int32_t *>(ws.d_stage.get() + o_flags);
        if (ws.timing) RC_HIP(hipEventRecord(ws.t0, s));
        pngz::png_inflate_kernel<<<n, pngz::LANES, 0, s>>>(reinterpret_cast<const uint32_t *>(ws.d_stage.get()),
                                                          reinterpret_cast<const pngz::IDesc *>(ws.d_stage.get()), ws.d_scan.get(),
                                                          d_flags);
        RC_LAUNCH_CHECK();
        if (ws.timing) RC_HIP(hipEventRecord(ws.t1, s));
        RC_HIP(hipMemcpyAsync(ws.h_flags.get(), d_flags, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        RC_HIP(hipStreamSynchronize(s));
        if (ws.timing) {
            float ms = 0.f;
            RC_HIP(hipEventElapsedTime(&ms, ws.t0, ws.t1));
            ws.kernel_ms += ms;
            ++ws.kernel_launches;
        }
        // reconstruct every run of images the device accepted; the others are the caller's
        const auto *d_rdesc = reinterpret_cast<const png::Desc *>(ws.d_stage.get() + o_rdesc);
        for (int i = 0; i < n;) {
            if (ws.h_flags.get()[i]) {
                flags_out[i++] = 1;
                ++ws.host_fallbacks;
                continue;
            }
            int e = i;
            while (e < n && !ws.h_flags.get()[e]) flags_out[e++] = 0;
            png::launch_reconstruct(ws.d_scan.get(), d_rdesc + i, reinterpret_cast<const uint32_t *>(ws.d_stage.get() + o_pal), rgb,
                                    e - i, s);
            ws.device_images += e - i;
            i = e;
        }
        RC_HIP(hipEventRecord(ws.done, s));
    });
}

extern "C" int rc_png_decode_stats(int device, int64_t *device_images, int64_t *host_fallbacks) {
    return guard([&] {
        RC_REQUIRE(device_images && host_fallbacks, RC_ERR_INVALID, "null argument");
        pngz::Workspace &ws = pngz::workspace(device);
        std::lock_guard<std::mutex> lock(ws.mu);
        *device_images = ws.device_images;
        *host_fallbacks = ws.host_fallbacks;
    });
}

extern "C" int rc_png_decode_timing(int device, int enable, double *kernel_ms, int64_t *launches) {
    return guard([&] {
        pngz::Workspace &ws = pngz::workspace(device);
        std::lock_guard<std::mutex> lock(ws.mu);
        if (enable && !ws.t0) {
            DeviceScope ds(device);
            RC_HIP(hipEventCreate(&ws.t0));
            RC_HIP(hipEventCreate(&ws.t1));
        }
        ws.timing = enable != 0;
        if (kernel_ms) *kernel_ms = ws.kernel_ms;
        if (launches) *launches = ws.kernel_launches;
        ws.kernel_ms = 0.0;
        ws.kernel_launches = 0;
    });
}
