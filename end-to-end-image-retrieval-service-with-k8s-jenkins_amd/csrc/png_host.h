// png_host.h — what png.hip (reconstruction) and png_inflate.hip (device inflate) share: the
// reconstruction kernel's descriptor and limits, the checks of an image's header fields, and the
// launch of png_reconstruct_kernel.
#pragma once

#include <algorithm>
#include <string>

#include "rc_common.h"

namespace rc {
namespace png {

constexpr int kMaxUnits = 3072;   // widest row in filter units (carry row in LDS)
constexpr int64_t kMaxPixels = 1 << 24;          // largest image (png.py MAX_PIXELS)
constexpr size_t kMaxStageBytes = 512u << 20;    // the staging of one call, so how far it grows

struct Desc {
    int64_t in_off;   // filtered scanlines in the staging block
    int64_t out_off;  // HWC RGB output, bytes from the output base
    int32_t width, height;
    int32_t stride;  // data bytes per scanline (without the filter byte)
    int32_t bpp;     // filter unit, bytes
    int32_t depth;   // bits per sample
    int32_t color;   // PNG colour type 0, 2, 3, 4, 6
    int32_t pal_off; // palette (256 packed 0x00BBGGRR entries) in the palette table, or -1
    int32_t pad;
};

inline int channels_of(int color) { return color == 2 ? 3 : color == 4 ? 2 : color == 6 ? 4 : 1; }

// The header fields of an rc_png_image or rc_png_stream, checked on the host before any device
// call; returns the data bytes of a scanline.
template <class T>
int64_t check_header(const T &p, const std::string &id) {
    RC_REQUIRE(p.width >= 1 && p.height >= 1 && p.width <= kMaxPixels && p.height <= kMaxPixels, RC_ERR_INVALID,
               id + "bad size");
    RC_REQUIRE((int64_t)p.width * p.height <= kMaxPixels, RC_ERR_UNSUPPORTED, id + "more than 2^24 pixels");
    const bool sub8 = p.depth == 1 || p.depth == 2 || p.depth == 4;
    const bool ok = (p.color == 0 || p.color == 3) ? (sub8 || p.depth == 8)
                                                   : ((p.color == 2 || p.color == 4 || p.color == 6) && p.depth == 8);
    RC_REQUIRE(ok, p.depth == 16 ? RC_ERR_UNSUPPORTED : RC_ERR_INVALID, id + "colour type / bit depth not handled");
    const int64_t bits = (int64_t)p.depth * channels_of(p.color);
    const int64_t stride = ((int64_t)p.width * bits + 7) / 8;
    const int bpp = (int)std::max<int64_t>(1, bits / 8);
    RC_REQUIRE(stride / bpp <= kMaxUnits, RC_ERR_UNSUPPORTED, id + "row wider than the carry row in LDS");
    return stride;
}

template <class T>
void check_palette_and_output(const T &p, const std::string &id, int64_t rgb_bytes) {
    if (p.color == 3)
        RC_REQUIRE(p.palette && p.palette_entries >= 1 && p.palette_entries <= 256, RC_ERR_INVALID,
                   id + "indexed image without a palette of 1..256 entries");
    RC_REQUIRE(p.out_offset >= 0 && p.out_offset + (int64_t)p.width * p.height * 3 <= rgb_bytes, RC_ERR_INVALID,
               id + "output range outside the buffer");
}

// Fill the reconstruction descriptor of one image and, for an indexed one, its palette slot
// (entries past PLTE are black, as Pillow's palette has them).
template <class T>
void fill_desc(Desc &d, const T &p, int64_t in_off, uint32_t *pal, int &ipal) {
    const int64_t bits = (int64_t)p.depth * channels_of(p.color);
    d.in_off = in_off;
    d.out_off = p.out_offset;
    d.width = p.width, d.height = p.height;
    d.stride = (int32_t)(((int64_t)p.width * bits + 7) / 8);
    d.bpp = (int32_t)std::max<int64_t>(1, bits / 8);
    d.depth = p.depth, d.color = p.color;
    d.pal_off = -1, d.pad = 0;
    if (p.color == 3) {
        d.pal_off = ipal * 256;
        uint32_t *q = pal + d.pal_off;
        for (int e = 0; e < 256; ++e)
            q[e] = e < p.palette_entries ? (uint32_t)p.palette[3 * e] | (uint32_t)p.palette[3 * e + 1] << 8 |
                                               (uint32_t)p.palette[3 * e + 2] << 16
                                         : 0u;
        ++ipal;
    }
}

// n blocks of png_reconstruct_kernel on s (png.hip).
void launch_reconstruct(const uint8_t *stage, const Desc *descs, const uint32_t *palettes, uint8_t *out, int n,
                        hipStream_t s);

}  // namespace png
}  // namespace rc
