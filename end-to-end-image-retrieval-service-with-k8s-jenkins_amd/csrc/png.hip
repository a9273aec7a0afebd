// png.hip — PNG reconstruction (un-filtering) and expansion to HWC RGB u8 on gfx950.
//
// The host has parsed the chunks and inflated IDAT (png.py); what arrives here is, per image, the
// filtered scanlines (H rows of one filter byte + `stride` data bytes) and a validated descriptor.
// rc_png_reconstruct copies the scanlines of a whole batch into one pinned staging block, uploads
// it with one copy and runs ONE kernel launch: a block per image.
//
// Wavefront.  A filter unit is bpp bytes (1 for gray / palette / packed samples, 2 gray+alpha,
// 3 RGB, 4 RGBA) and is kept packed in one VGPR.  Unit x of row r needs unit x-1 of row r (a) and
// units x (b) and x-1 (c) of row r-1; Average and Paeth are not associative, so rows cannot be
// scanned.  One lane owns one row of a 64-row band and runs one unit behind the lane above it: at
// step t lane l reconstructs unit t-l.  Then b is what lane l-1 produced one step ago — one DPP
// wave_shr:1 of the previous result — and c is the b of the step before; neither is read from
// memory.  Lane 0 takes its b from the carry row (the last row of the band above) kept in LDS.
// The four byte lanes of a unit are split into even and odd bytes held in 16-bit fields
// (0x00FF00FF), so the Paeth distances, the Average sum and the final add run as packed 16-bit
// operations on two bytes at a time and the three-way Paeth choice is two sign masks and two
// bit-selects; no byte ever carries into its neighbour.
//
// Waves and phases.  Time is cut into phases of T = 64 steps, with block barriers between them and
// nowhere else.  The kNW waves of a block take consecutive bands; wave w starts 2 phases after
// wave w-1, because unit x of a band's last row (lane 63) exists at step x+63 and the band below
// reads it at its own step x: 2T >= T+63 puts the write at least one barrier before the read.
// After its band a wave takes band +kNW; a round lasts R = max(P, 2 kNW, 3) phases (P = phases
// per band), which keeps (a) a wave's rounds apart, (b) wave kNW-1's carry ahead of wave 0's next
// band and (c) a carry row from being overwritten before the band below has read it.  Every wave
// runs every phase and every barrier; a wave outside its window only idles.  All trip counts come
// from the descriptor (W, H, bpp, depth); no loop or branch bound is read from the stream's
// bytes, and there is no waiting on memory.  A filter byte above 4 (the host refuses those) would
// act as None.
//
// LDS.  Per wave one tile of 64 rows x 64 units, a dword per unit, row pitch 65 dwords, skewed the
// way the wavefront walks it: slot (l, s) of phase p holds unit 64p + s - l of row l.
//   * load: for each row the 64 lanes fetch the 64 consecutive units of its slice (byte loads,
//     64*bpp consecutive bytes per row) and write 64 consecutive dwords: no conflict.  Eight rows
//     are fetched at a time, branch-free, so that their loads overlap: one wave per SIMD has
//     nothing else to hide a load's latency behind.
//   * wavefront: at step s lane l reads and rewrites dword l*65 + s, bank (l + s) mod 64: the 64
//     lanes fall on 64 different banks — the pitch of 65 is the padding that makes the transposed
//     access conflict-free (a pitch of 64 would put all lanes on one bank).
//   * store: per row the lanes read 64 consecutive dwords again and write the row's slice as RGB,
//     64*3 consecutive bytes for the 8-bit types (more pixels per unit for depths 1, 2, 4).
// The tile is reused in place (filtered in, reconstructed out).  Besides the tiles: one carry row
// per wave (kMaxUnits dwords; wider rows are RC_ERR_UNSUPPORTED) and a 256-entry palette copy.
//   kNW = 2:  2 * 64*65*4 + 2 * 3072*4 + 1024 = 58,880 B of the 64 KiB a block may take statically.
#include <algorithm>
#include <vector>

#include "png_host.h"

namespace rc {
namespace png {

constexpr int kNW = 2;            // waves (bands in flight) per block
constexpr int kT = 64;            // steps per phase = units per tile row
constexpr int kPitch = kT + 1;    // tile row pitch in dwords (odd: conflict-free transposed access)
constexpr int kLag = 2;           // phases wave w runs behind wave w-1 (kLag * kT >= kT + 63)

typedef short short2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t as_u32(short2_t v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ short2_t as_s2(uint32_t v) { return __builtin_bit_cast(short2_t, v); }

// Predictor of two bytes held in 16-bit fields.  sel_*: all-ones masks of this lane's filter type.
__device__ __forceinline__ uint32_t predict(uint32_t a, uint32_t b, uint32_t c, uint32_t sel_a, uint32_t sel_b,
                                            uint32_t sel_avg, uint32_t sel_paeth) {
    const short2_t sa = as_s2(a), sb = as_s2(b), sc = as_s2(c);
    const short2_t db = sb - sc, da = sa - sc;  // p - a, p - b  with p = a + b - c
    const short2_t dc = db + da;                // p - c
    const short2_t pa = __builtin_elementwise_max(db, -db);
    const short2_t pb = __builtin_elementwise_max(da, -da);
    const short2_t pc = __builtin_elementwise_max(dc, -dc);
    // a unless pa > min(pb, pc); otherwise b unless pb > pc; otherwise c
    const uint32_t not_a = as_u32((__builtin_elementwise_min(pb, pc) - pa) >> 15);
    const uint32_t not_b = as_u32((pc - pb) >> 15);
    const uint32_t bc = (c & not_b) | (b & ~not_b);
    const uint32_t paeth = (bc & not_a) | (a & ~not_a);
    const uint32_t avg = ((a + b) >> 1) & 0x00FF00FFu;  // 9-bit sums: the fields cannot touch
    return (a & sel_a) | (b & sel_b) | (avg & sel_avg) | (paeth & sel_paeth);
}

__global__ __launch_bounds__(64 * kNW) void png_reconstruct_kernel(const uint8_t *__restrict__ stage,
                                                                   const Desc *__restrict__ descs,
                                                                   const uint32_t *__restrict__ palettes,
                                                                   uint8_t *__restrict__ out) {
    __shared__ uint32_t tile[kNW][kT * kPitch];
    __shared__ uint32_t carry[kNW][kMaxUnits];
    __shared__ uint32_t pal[256];

    const Desc d = descs[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = d.width, H = d.height, stride = d.stride, bpp = d.bpp, depth = d.depth;
    const int U = stride / bpp;                  // filter units per row
    const int P = (U + 63 + kT - 1) / kT;        // phases per band
    const int bands = (H + 63) / 64;
    const int rounds = (bands + kNW - 1) / kNW;
    const int R = max(P, max(2 * kNW, 3));
    const int phases = rounds * R + kLag * (kNW - 1);
    const int ppu = (depth < 8) ? 8 / depth : 1;  // pixels per unit
    const uint32_t smask = (1u << depth) - 1u;    // depth <= 8
    const bool indexed = d.color == 3, gray = d.color == 0 || d.color == 4;
    const uint32_t gscale = 255u / smask;         // Pillow's L;1 / L;2 / L;4 scaling (x255, x85, x17)
    const uint8_t *src = stage + d.in_off;
    uint8_t *dst = out + d.out_off;
    const int64_t pitch_in = (int64_t)stride + 1;

    for (int i = threadIdx.x; i < 256; i += 64 * kNW) pal[i] = indexed ? palettes[d.pal_off + i] : 0u;
    uint32_t *mytile = tile[wave];
    const uint32_t *prev_carry = carry[(wave + kNW - 1) % kNW];
    uint32_t *my_carry = carry[wave];

    // wavefront state of this lane's row: previous result (a), previous up (becomes c)
    uint32_t res = 0, up_e = 0, up_o = 0, a_e = 0, a_o = 0;
    uint32_t sel_a = 0, sel_b = 0, sel_avg = 0, sel_paeth = 0;

    for (int g = 0; g < phases; ++g) {
        const int local = g - kLag * wave;
        const int round = local >= 0 ? local / R : 0;
        const int ph = local >= 0 ? local - round * R : 0;
        const int band = round * kNW + wave;
        const bool active = local >= 0 && ph < P && band < bands;  // wave-uniform
        const int row = band * 64 + lane;
        const int t0 = ph * kT;  // first step of the phase

        __syncthreads();  // the phase boundary: carries written last phase, the palette copy
        if (active) {
            if (ph == 0) {
                res = up_e = up_o = a_e = a_o = 0;
                const int ft = row < H ? src[row * pitch_in] : 0;
                sel_a = ft == 1 ? ~0u : 0u;
                sel_b = ft == 2 ? ~0u : 0u;
                sel_avg = ft == 3 ? ~0u : 0u;
                sel_paeth = ft == 4 ? ~0u : 0u;
            }
            // ---- load: row rr's slice, units t0 - rr .. t0 - rr + 63, one unit per lane
            const int rows_here = min(64, H - band * 64);
            // eight rows at a time: their byte loads are all in flight before the first LDS write
            for (int r0 = 0; r0 < rows_here; r0 += 8) {
                uint32_t v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int rr = r0 + k, u = t0 - rr + lane;
                    // branch-free so that the loads can be batched: a slot outside the row reads the
                    // image's first bytes instead (1 + bpp of them exist) and is zeroed
                    const bool ok = rr < rows_here && u >= 0 && u < U;
                    const uint8_t *p = ok ? src + (int64_t)(band * 64 + rr) * pitch_in + 1 + (int64_t)u * bpp : src;
                    const uint32_t b0 = p[0], b1 = p[min(1, bpp - 1)], b2 = p[min(2, bpp - 1)], b3 = p[min(3, bpp - 1)];
                    const uint32_t w = b0 | (bpp > 1 ? b1 << 8 : 0u) | (bpp > 2 ? b2 << 16 : 0u) | (bpp > 3 ? b3 << 24 : 0u);
                    v[k] = ok ? w : 0u;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k)  // rows past rows_here: zeros into rows of the tile nobody reads out
                    mytile[(r0 + k) * kPitch + lane] = v[k];
            }
        }
        __syncthreads();
        if (active) {
            // ---- wavefront: 64 steps, every lane in every step (the DPP shift reads all lanes)
            const bool row_ok = row < H;
            for (int s = 0; s < kT; ++s) {
                const int x = t0 + s - lane;
                const bool valid = row_ok && x >= 0 && x < U;
                const uint32_t f = mytile[lane * kPitch + s];
                uint32_t above = 0;  // lane 0: the band above's last row
                if (lane == 0 && band > 0 && valid) above = prev_carry[x];
                const uint32_t b = __builtin_amdgcn_update_dpp(above, res, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
                const uint32_t b_e = b & 0x00FF00FFu, b_o = (b >> 8) & 0x00FF00FFu;
                const uint32_t p_e = predict(a_e, b_e, up_e, sel_a, sel_b, sel_avg, sel_paeth);
                const uint32_t p_o = predict(a_o, b_o, up_o, sel_a, sel_b, sel_avg, sel_paeth);
                const uint32_t r_e = valid ? ((f & 0x00FF00FFu) + p_e) & 0x00FF00FFu : 0u;
                const uint32_t r_o = valid ? (((f >> 8) & 0x00FF00FFu) + p_o) & 0x00FF00FFu : 0u;
                res = r_e | (r_o << 8);
                a_e = r_e, a_o = r_o;
                up_e = b_e, up_o = b_o;
                mytile[lane * kPitch + s] = res;
                if (lane == 63 && valid) my_carry[x] = res;
            }
        }
        __syncthreads();
        if (active) {
            // ---- store: row rr's slice as RGB, one unit per lane
            const int rows_here = min(64, H - band * 64);
            for (int rr = 0; rr < rows_here; ++rr) {
                const int u = t0 - rr + lane;
                if (u < 0 || u >= U) continue;
                const uint32_t v = mytile[rr * kPitch + lane];
                uint8_t *o = dst + ((int64_t)(band * 64 + rr) * W) * 3;
                for (int j = 0; j < ppu; ++j) {
                    const int px = u * ppu + j;
                    if (px >= W) break;
                    const uint32_t smp = (v >> (8 - depth * (j + 1))) & smask;  // depth 8: the unit's byte 0
                    const uint32_t rgb = indexed ? pal[smp] : gray ? smp * gscale * 0x010101u : v;
                    o[px * 3 + 0] = (uint8_t)rgb;
                    o[px * 3 + 1] = (uint8_t)(rgb >> 8);
                    o[px * 3 + 2] = (uint8_t)(rgb >> 16);
                }
            }
        }
    }
}

// Per-device staging, grown geometrically and reused: pinned host block, its device copy, and the
// event of the last upload out of the pinned block (a later call waits for it before refilling)
// and of the last kernel (a later call's stream waits for it before overwriting the device copy).
struct Workspace {
    std::mutex mu;
    PinBuf<uint8_t> h_stage;
    DevBuf<uint8_t> d_stage;
    hipEvent_t staged = nullptr, done = nullptr;
};

static Workspace &workspace(int device) {
    static Workspace *const ws = new Workspace[64];  // never destroyed: no device call runs at process exit
    RC_REQUIRE(device >= 0 && device < 64, RC_ERR_INVALID, "device ordinal out of range");
    return ws[device];
}

// Everything the kernel's bounds rest on, checked on the host before any device call.
static void validate(int n, const rc_png_image *im, const uint8_t *rgb, int64_t rgb_bytes) {
    RC_REQUIRE(n >= 1 && n <= 65535, RC_ERR_INVALID, "image count must be 1..65535");
    RC_REQUIRE(im && rgb && rgb_bytes > 0, RC_ERR_INVALID, "null argument");
    for (int i = 0; i < n; ++i) {
        const rc_png_image &p = im[i];
        const std::string id = "image " + std::to_string(i) + ": ";
        const int64_t stride = check_header(p, id);
        RC_REQUIRE(p.scanlines && p.scan_bytes == (int64_t)p.height * (1 + stride), RC_ERR_INVALID,
                   id + "scanline bytes are not height * (1 + stride)");
        for (int64_t r = 0; r < p.height; ++r)
            RC_REQUIRE(p.scanlines[r * (1 + stride)] <= 4, RC_ERR_INVALID, id + "filter byte above 4");
        check_palette_and_output(p, id, rgb_bytes);
    }
}

void launch_reconstruct(const uint8_t *stage, const Desc *descs, const uint32_t *palettes, uint8_t *out, int n,
                        hipStream_t s) {
    png_reconstruct_kernel<<<n, 64 * kNW, 0, s>>>(stage, descs, palettes, out);
    RC_LAUNCH_CHECK();
}

}  // namespace png
}  // namespace rc

using namespace rc;

extern "C" int rc_png_reconstruct(int device, int n, const rc_png_image *images, uint8_t *rgb, int64_t rgb_bytes,
                                  void *stream) {
    return guard([&] {
        png::validate(n, images, rgb, rgb_bytes);
        auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
        // staging layout: descriptors | palettes (1 KiB each) | scanlines (256-B aligned per image)
        int npal = 0;
        for (int i = 0; i < n; ++i) npal += images[i].color == 3;
        const size_t o_pal = al((size_t)n * sizeof(png::Desc));
        const size_t o_scan = o_pal + (size_t)npal * 1024;
        size_t total = o_scan;
        for (int i = 0; i < n; ++i) total += al((size_t)images[i].scan_bytes);
        RC_REQUIRE(total <= png::kMaxStageBytes, RC_ERR_UNSUPPORTED,
                   "the scanlines of one call exceed the 512 MiB staging cap: split the batch");

        png::Workspace &ws = png::workspace(device);
        std::lock_guard<std::mutex> lock(ws.mu);
        DeviceScope ds(device);
        if (!ws.staged) RC_HIP(hipEventCreateWithFlags(&ws.staged, hipEventDisableTiming));
        if (!ws.done) RC_HIP(hipEventCreateWithFlags(&ws.done, hipEventDisableTiming));
        RC_HIP(hipEventSynchronize(ws.staged));  // the last upload has left the pinned block
        if (const size_t cap = min_capacity(ws.h_stage, ws.d_stage); total > cap) {
            const size_t want = std::min(std::max(total, cap * 2), png::kMaxStageBytes);
            RC_HIP(hipDeviceSynchronize());  // a kernel may still read the old device copy
            ws.h_stage.reserve(want);
            ws.d_stage.reserve(want);
        }
        auto *desc = reinterpret_cast<png::Desc *>(ws.h_stage.get());
        auto *pal = reinterpret_cast<uint32_t *>(ws.h_stage.get() + o_pal);
        size_t at = o_scan;
        int ipal = 0;
        for (int i = 0; i < n; ++i) {
            const rc_png_image &p = images[i];
            png::fill_desc(desc[i], p, (int64_t)at, pal, ipal);
            std::memcpy(ws.h_stage.get() + at, p.scanlines, (size_t)p.scan_bytes);
            at += al((size_t)p.scan_bytes);
        }
        hipStream_t s = (hipStream_t)stream;
        RC_HIP(hipStreamWaitEvent(s, ws.done, 0));
        RC_HIP(hipMemcpyAsync(ws.d_stage.get(), ws.h_stage.get(), total, hipMemcpyHostToDevice, s));
        RC_HIP(hipEventRecord(ws.staged, s));
        png::launch_reconstruct(ws.d_stage.get(), reinterpret_cast<png::Desc *>(ws.d_stage.get()),
                                reinterpret_cast<uint32_t *>(ws.d_stage.get() + o_pal), rgb, n, s);
        RC_HIP(hipEventRecord(ws.done, s));
    });
}
