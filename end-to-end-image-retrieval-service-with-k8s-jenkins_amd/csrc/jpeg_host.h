// jpeg_host.h — what jpeg.hip (marker parse, host Huffman, reconstruction) and
// jpeg_entropy.hip (the device entropy stage) share: the parsed header and the
// entropy stage's host interface.
#pragma once

#include <cstdint>
#include <string>

#include "rc_common.h"

namespace rc {
namespace jpeg {

struct Huff {
    bool present = false;
    // canonical decoding: maxcode[l] (codes of length l are < maxcode[l]),
    // valptr[l] - mincode[l] indexes vals; a 9-bit lookahead table for speed
    int32_t maxcode[18];
    int32_t delta[17];
    uint8_t vals[256];
    uint16_t look[512];  // (length << 8) | value, length 0 = not in table
};

struct Comp {
    int id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0;
    int bw = 0, bh = 0;  // blocks per plane (MCU padded)
    int64_t blk0 = 0;    // first block of the plane within the image
};

struct Header {
    int width = 0, height = 0, ncomp = 0, hmax = 1, vmax = 1, restart = 0, mcux = 0, mcuy = 0;
    Comp c[3];
    uint16_t qt[4][64];
    bool qt_present[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    const uint8_t *scan = nullptr;
    const uint8_t *end = nullptr;
    int scan_ncomp = 0, scan_comp[3] = {0, 0, 0};
    bool jfif = false, adobe = false;
    int adobe_transform = -1;
    int64_t blocks = 0;
    bool supported = false;
    std::string why;
};

// ---------------------------------------------------------------------------
// Device entropy stage (jpeg_entropy.hip).  A call goes begin -> prepare (per
// image, from any thread) -> decode.  `staging` is the pinned coefficient
// staging of the call (nb × 128 B).  begin gives every image a slice of it, back
// to back, as large as its segment table and scan can get (never more than its
// coefficients would take); prepare writes the table and the unstuffed scan
// there.  prepare returns false for an image the device stage does not take
// (the caller decodes it on the host); decode uploads the slices with one copy,
// runs the kernels, writes quantised coefficients (with the DC prediction
// applied) into d_coef, and returns one flag per image in flags[]: nonzero =
// not decoded here, the host decoder has the say.  It returns the bytes it
// uploaded.
struct EntropyWork;
EntropyWork *entropy_create(int max_images, int64_t max_blocks);
void entropy_destroy(EntropyWork *w);
void entropy_begin(EntropyWork *w, int n, const Header *hd);
bool entropy_prepare(EntropyWork *w, int i, const Header &hd, int64_t blk_base, uint8_t *staging);
size_t entropy_decode(EntropyWork *w, int n, int64_t nb, const uint8_t *staging, int16_t *d_coef, hipStream_t s,
                      int32_t *flags);

}  // namespace jpeg
}  // namespace rc
