// jpeg_entropy.hip — the JPEG entropy stage on the GPU: baseline Huffman scans decoded by
// self-synchronising subsequence decoders, into the same quantised coefficients (int16, natural
// order, planes in component order) that jpeg.hip's host decoder produces.  DESIGN.md "JPEG
// entropy decode on the device".
//
// Host (entropy_prepare, per image): the scan is copied into the pinned staging with the stuffed
// 0x00 bytes removed, cut at its restart markers (each checked against RST0..7 in order, as
// Bits::restart does), every segment as big-endian dwords on a 4-byte boundary, behind a table of
// {offset, bits, first lane}.  A segment is cut into subsequences of SUB_BITS bits, one lane each;
// lanes are numbered through the image's segments and grouped LANES to a workgroup.
//
// Device, per batch:
//   jpeg_entropy_sync_kernel   one workgroup per group of LANES subsequences.  The group's rows of
//       the scan and the image's Huffman tables are staged in LDS; every lane decodes its row
//       from a guessed state (slot 0, k 0, bit 0), writing nothing but its exit state, then
//       takes its left neighbour's exit as its entry and decodes again until no exit changes
//       (at most LANES rounds: after round j the first j lanes are right).  Launched
//       SYNC_PASSES times when a segment spans groups: pass r hands group g the exit that group
//       g - 1 reached in pass r - 1; a group whose entry did not change copies one word.
//   jpeg_entropy_write_kernel  checks that every group's entry is its left group's final exit (by
//       induction from the segment's first lane, whose state is known, every lane's then is the
//       true decoder's), turns the lanes' block counts into block ordinals with a block scan, and
//       decodes once more from the true states, storing AC values and DC differences and raising
//       the image's flag at anything the host decoder would refuse.
//   jpeg_dc_kernel             per component, the running sum of the DC differences in scan
//       order, restarted at every restart interval: the host's `pred`.
//
// The stream's bits select values only: every loop bound and address comes from the descriptor
// the host built, positions and states are clamped, ordinals are tested before a store.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "jpeg_host.h"

namespace rc {
namespace jpeg {

constexpr int SUB_BITS = RC_JPEG_ENTROPY_SUBSEQ_BITS;   // bits of one lane's subsequence
constexpr int SUB_DW = SUB_BITS / 32;
constexpr int LANES = RC_JPEG_ENTROPY_GROUP_LANES;      // subsequences per workgroup
// a symbol that starts inside the row reads 32 bits from there: one dword past the row; the row
// pitch is odd, so the lanes' reads at a common column fall into different banks
constexpr int ROW_DW = SUB_DW + 1;
static_assert(ROW_DW % 2 == 1, "odd LDS row pitch");
constexpr int SYNC_PASSES = 4;  // launches of the sync kernel when a segment spans groups
constexpr int MAX_SLOTS = 10;   // blocks per MCU (the standard's limit)

__device__ static const uint8_t kZigzagDev[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                                  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                                  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                                  58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// One Huffman table in the host decoder's own form (Huff): the 9-bit lookahead, and maxcode /
// delta for the code lengths 10..16.
struct Tab {
    uint16_t look[512];
    int32_t maxcode[7], delta[7];
    uint8_t vals[256];
};

struct EDesc {
    int32_t nlanes, nseg, nslots, mcux;
    int32_t nmcu, interval, lane_base, ncomp;  // interval: MCUs per segment (all of them without DRI)
    int64_t region_off;                        // the image's segment table + scan, bytes into the upload
    int64_t coef_base;                         // the image's first block in d_coef
    int32_t blocks, pad0;
    int32_t ch[3], cv[3], cbw[3], cblk0[3];
    uint8_t slot_comp[12], slot_v[12], slot_h[12];
    Tab tab[6];  // [2c] component c's DC table, [2c + 1] its AC table
};
static_assert(sizeof(EDesc) % 8 == 0, "EDesc is copied as dwords");

struct Seg {
    uint32_t off, nbits, lane0, pad;  // byte offset within the region (4-aligned), bits, first lane
};

struct GroupEnt {
    int32_t img, lane0;  // first lane (within the image)
    int32_t chained;     // the first lane continues a segment begun in an earlier group
    int32_t gfirst;      // then: the group that holds that segment's first lane
};

struct GroupLds {
    uint32_t row[LANES * ROW_DW];
    EDesc e;
    uint32_t ex[LANES];   // exit states (sync) / exclusive block counts (write)
    uint32_t src[LANES];  // a row's first dword in the region
    int32_t ndw[LANES];   // dwords of it that exist
    uint32_t wsum[LANES / 64];
    uint32_t misc[4];
};

struct LaneInfo {
    bool active, first, last_row, last_seg;
    int seg, sub, lim;
    uint32_t nbits, lane0;
};

// state word: bit offset past the row's end (0..31) | slot << 5 | k << 9
__device__ __forceinline__ uint32_t pack_state(int poff, int slot, int k) {
    return (uint32_t)poff | ((uint32_t)slot << 5) | ((uint32_t)k << 9);
}

__device__ __forceinline__ bool lookup(const Tab &t, uint32_t v, int &len, int &sym) {
    const uint32_t e = t.look[v >> 23];
    if (e) {
        len = max((int)(e >> 8) & 15, 1);
        sym = (int)(e & 0xFF);
        return true;
    }
    const int code = (int)(v >> 16);
#pragma unroll
    for (int l = 10; l <= 16; ++l) {
        const int c = code >> (16 - l);
        if (c < t.maxcode[l - 10]) {
            const int idx = c + t.delta[l - 10];
            if ((unsigned)idx > 255u) return false;
            len = l;
            sym = t.vals[idx];
            return true;
        }
    }
    return false;
}

// Stage the group in LDS: the image's descriptor, and each lane's row of its segment (dwords past
// the segment's end read as zero, the host decoder's fill).  Returns this lane's place.
__device__ __forceinline__ LaneInfo group_setup(GroupLds &L, const EDesc *__restrict__ descs, const GroupEnt &ge,
                                                const uint8_t *__restrict__ ent) {
    const int tid = (int)threadIdx.x;
    {
        const uint32_t *s = reinterpret_cast<const uint32_t *>(descs + ge.img);
        uint32_t *d = reinterpret_cast<uint32_t *>(&L.e);
        for (int i = tid; i < (int)(sizeof(EDesc) / 4); i += LANES) d[i] = s[i];
    }
    __syncthreads();
    const EDesc &e = L.e;
    const uint8_t *region = ent + e.region_off;
    const Seg *segs = reinterpret_cast<const Seg *>(region);
    LaneInfo li;
    const int l = ge.lane0 + tid;
    li.active = l < e.nlanes;
    li.seg = 0;
    li.sub = 0;
    li.nbits = 0;
    li.lane0 = 0;
    uint32_t off = 0;
    if (li.active) {
        int lo = 0, hi = e.nseg;  // the last segment whose first lane is <= l
        for (int it = 0; it < 32 && hi - lo > 1; ++it) {
            const int mid = (lo + hi) >> 1;
            if (segs[mid].lane0 <= (uint32_t)l) lo = mid;
            else hi = mid;
        }
        const Seg sg = segs[lo];
        li.seg = lo;
        li.lane0 = sg.lane0;
        li.sub = l - (int)sg.lane0;
        li.nbits = sg.nbits;
        off = sg.off;
    }
    const int seg_dw = (int)((li.nbits + 31u) >> 5);
    const int64_t rel = (int64_t)li.nbits - (int64_t)li.sub * SUB_BITS;  // bits of the segment from this row on
    li.lim = li.active ? (int)(rel < 0 ? 0 : (rel > SUB_BITS ? SUB_BITS : rel)) : 0;
    li.first = li.sub == 0;
    li.last_row = rel <= SUB_BITS;
    li.last_seg = li.seg == e.nseg - 1;
    L.src[tid] = (off >> 2) + (uint32_t)li.sub * SUB_DW;
    L.ndw[tid] = li.active ? max(0, seg_dw - li.sub * SUB_DW) : 0;
    __syncthreads();
    const uint32_t *r32 = reinterpret_cast<const uint32_t *>(region);
    for (int idx = tid; idx < LANES * ROW_DW; idx += LANES) {
        const int r = idx / ROW_DW, c = idx - r * ROW_DW;
        L.row[idx] = c < L.ndw[r] ? r32[L.src[r] + c] : 0u;
    }
    __syncthreads();
    return li;
}

// What the write pass needs beyond the state.
struct WriteCtx {
    int16_t *coef;     // the image's first block
    int32_t *flag;     // the image's flag
    uint32_t ord;      // blocks of the segment begun before this lane
    uint32_t expected; // blocks of the segment
    int mcu0;          // the segment's first MCU
};

__device__ __forceinline__ int16_t *block_ptr(const EDesc &e, const WriteCtx &w, uint32_t ord) {
    const int m = w.mcu0 + (int)(ord / (uint32_t)e.nslots), sl = (int)(ord % (uint32_t)e.nslots);
    const int c = e.slot_comp[sl] % 3;
    const int my = m / e.mcux, mx = m - my * e.mcux;
    const int b = e.cblk0[c] + (my * e.cv[c] + e.slot_v[sl]) * e.cbw[c] + mx * e.ch[c] + e.slot_h[sl];
    if ((unsigned)b >= (unsigned)e.blocks) return nullptr;
    return w.coef + (int64_t)b * 64;
}

// Decode the symbols that start inside one row, from `entry`.  WRITE = false: nothing is stored;
// an invalid code takes one bit, a run past 63 ends the block, any DC size is taken (low 4
// bits): wrong states meet these all the time.  WRITE = true (true states): each is the host
// decoder's error and raises the flag, as do a block the segment has no room for and a segment
// that does not end where its blocks do.
template <bool WRITE>
__device__ __forceinline__ void decode_row(const EDesc &e, const uint32_t *row, const LaneInfo &li, uint32_t entry,
                                           uint32_t &exitv, uint32_t &begun, WriteCtx w) {
    int p = (int)(entry & 31u), slot = (int)((entry >> 5) & 15u), k = (int)((entry >> 9) & 63u);
    if (slot >= e.nslots) slot = 0;
    uint32_t n = 0;
    int16_t *blk = nullptr;  // the block being written (null: none, or one past the segment's count)
    if (WRITE && k > 0 && w.ord >= 1 && w.ord - 1 < w.expected) blk = block_ptr(e, w, w.ord - 1);
    bool stop = false;
    while (p < li.lim) {  // every round consumes at least one bit
        if (WRITE && k == 0 && w.ord + n >= w.expected) {  // padding bits past the last block: not a block
            stop = true;
            break;
        }
        const int wd = p >> 5, sh = p & 31;
        const uint64_t q = ((uint64_t)row[wd] << 32) | row[wd + 1];
        const uint32_t v = (uint32_t)(q >> (32 - sh));
        const int c = e.slot_comp[slot] % 3;
        const Tab &t = e.tab[2 * c + (k ? 1 : 0)];
        int len = 1, sym = 0;
        const bool ok = lookup(t, v, len, sym);
        if (!ok) {
            if (WRITE && (blk || k == 0)) {
                *w.flag = 1;  // corrupt Huffman data
                return;
            }
            len = 1;
            sym = 0;
        }
        const int s = sym & 15, r = sym >> 4;
        int val = 0;
        if (s) {
            val = (int)((v << len) >> (32 - s));
            if (val < (1 << (s - 1))) val += 1 - (1 << s);
        }
        p += len + s;
        if (k == 0) {
            if (WRITE) {
                blk = block_ptr(e, w, w.ord + n);
                if (sym > 11 || !blk) {
                    *w.flag = 1;  // corrupt DC
                    return;
                }
                blk[0] = (int16_t)val;  // the difference; jpeg_dc_kernel sums them
            }
            ++n;
            k = 1;
        } else {
            if (s) {
                k += r;
                if (k > 63) {
                    if (WRITE && blk) {
                        *w.flag = 1;  // corrupt AC run
                        return;
                    }
                    k = 64;
                } else {
                    if (WRITE && blk) blk[kZigzagDev[k]] = (int16_t)val;
                    ++k;
                }
            } else {
                k = r == 15 ? k + 16 : 64;
            }
            if (k >= 64) {
                k = 0;
                slot = slot + 1 >= e.nslots ? 0 : slot + 1;
                if (WRITE && blk && w.ord + n == w.expected) {
                    // the segment's last block: it must end inside the segment (the host's
                    // overrun()), and in the last byte when a restart marker follows
                    const int64_t pos = (int64_t)li.sub * SUB_BITS + p;
                    if (pos > (int64_t)li.nbits || (!li.last_seg && (int64_t)li.nbits - pos >= 8)) *w.flag = 1;
                    stop = true;
                    break;
                }
                blk = nullptr;
            }
        }
    }
    if (WRITE && !stop && li.last_row) {
        // the segment ended: all its blocks must have
        const uint32_t o = w.ord + n;
        if (o < w.expected || (o == w.expected && k != 0)) *w.flag = 1;
    }
    begun = n;
    exitv = pack_state(p >= SUB_BITS ? min(p - SUB_BITS, 31) : 0, slot, k);
}

__global__ __launch_bounds__(LANES) void jpeg_entropy_sync_kernel(const EDesc *__restrict__ descs,
                                                                 const GroupEnt *__restrict__ groups,
                                                                 const uint8_t *__restrict__ ent, uint32_t *__restrict__ lexit,
                                                                 uint32_t *__restrict__ lcnt, uint32_t *__restrict__ gentry,
                                                                 uint32_t *__restrict__ gexit, uint32_t *__restrict__ gtail,
                                                                 int G, int pass) {
    __shared__ GroupLds L;
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const GroupEnt ge = groups[g];
    uint32_t *gx_cur = gexit + (size_t)(pass & 1) * G;
    const uint32_t *gx_prev = gexit + (size_t)((pass & 1) ^ 1) * G;
    uint32_t E = 0;  // the group's entry state: a guess in pass 0
    if (pass > 0) {  // (block-uniform)
        if (ge.chained) E = gx_prev[g - 1];
        if (!ge.chained || E == gentry[g]) {  // nothing new to decode from
            if (tid == 0) gx_cur[g] = gx_prev[g];
            return;
        }
    }
    const LaneInfo li = group_setup(L, descs, ge, ent);
    L.ex[tid] = 0;
    if (tid == 0) L.misc[0] = 0;
    __syncthreads();
    uint32_t used = 0xffffffffu, exitv = 0, cnt = 0;
    for (int it = 0; it <= LANES; ++it) {
        const uint32_t entry = li.first ? 0u : (tid == 0 ? E : L.ex[tid - 1]);
        __syncthreads();
        int changed = 0;
        if (li.active && entry != used) {
            decode_row<false>(L.e, L.row + tid * ROW_DW, li, entry, exitv, cnt, WriteCtx{});
            used = entry;
            changed = exitv != L.ex[tid];
            L.ex[tid] = exitv;
        }
        if (!__syncthreads_or(changed)) break;
    }
    if (li.active) {
        lexit[L.e.lane_base + ge.lane0 + tid] = exitv;
        lcnt[L.e.lane_base + ge.lane0 + tid] = cnt;
    }
    // blocks begun in the lanes of the last lane's segment: the next group's ordinals start there
    if (tid == LANES - 1) L.misc[1] = li.active ? (uint32_t)li.seg : 0xffffffffu;
    __syncthreads();
    if (li.active && (uint32_t)li.seg == L.misc[1]) atomicAdd(&L.misc[0], cnt);
    __syncthreads();
    if (tid == 0) {
        gentry[g] = E;
        gx_cur[g] = L.ex[LANES - 1];
        gtail[g] = L.misc[0];
    }
}

__global__ __launch_bounds__(LANES) void jpeg_entropy_write_kernel(const EDesc *__restrict__ descs,
                                                                  const GroupEnt *__restrict__ groups,
                                                                  const uint8_t *__restrict__ ent,
                                                                  const uint32_t *__restrict__ lexit,
                                                                  const uint32_t *__restrict__ lcnt,
                                                                  const uint32_t *__restrict__ gentry,
                                                                  const uint32_t *__restrict__ gexit_final,
                                                                  const uint32_t *__restrict__ gtail, int16_t *__restrict__ coef,
                                                                  int32_t *__restrict__ flags) {
    __shared__ GroupLds L;
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const GroupEnt ge = groups[g];
    const LaneInfo li = group_setup(L, descs, ge, ent);
    const EDesc &e = L.e;
    if (tid == 0) {
        L.misc[0] = 0;
        // the chain of entries: this group decoded from the exit its left neighbour ended with
        if (ge.chained && gentry[g] != gexit_final[g - 1]) flags[ge.img] = 1;
    }
    const int l = ge.lane0 + tid;
    const uint32_t entry = (li.active && !li.first) ? lexit[e.lane_base + l - 1] : 0u;
    const uint32_t cnt = li.active ? lcnt[e.lane_base + l] : 0u;
    // exclusive sum of the block counts over the group: a wave scan, then the waves' totals
    uint32_t x = cnt;
    const int wl = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (wl >= d) x += y;
    }
    if (wl == 63) L.wsum[wv] = x;
    __syncthreads();
    for (int j = 0; j < wv; ++j) x += L.wsum[j];
    L.ex[tid] = x - cnt;
    // blocks of this segment begun in earlier groups
    if (ge.chained) {
        uint32_t part = 0;
        for (int j = ge.gfirst + tid; j < g; j += LANES) part += gtail[j];
        if (part) atomicAdd(&L.misc[0], part);
    }
    __syncthreads();
    if (!li.active) return;
    WriteCtx w;
    w.coef = coef + e.coef_base * 64;
    w.flag = flags + ge.img;
    const int first_in_group = (int)li.lane0 - ge.lane0;
    w.ord = first_in_group >= 0 ? (x - cnt) - L.ex[first_in_group] : L.misc[0] + (x - cnt);
    w.mcu0 = li.seg * e.interval;
    const int left = e.nmcu - w.mcu0;
    w.expected = (uint32_t)(max(0, min(e.interval, left)) * e.nslots);
    uint32_t exitv, n;
    decode_row<true>(e, L.row + tid * ROW_DW, li, entry, exitv, n, w);
}

// grid (3, n): component blockIdx.x of image blockIdx.y; its blocks in scan order, LANES at a
// time with a carry: position 0 holds the DC difference and gets the prediction, an int32 sum
// restarted with each restart interval and stored as the host's (int16_t)pred.
__global__ __launch_bounds__(LANES) void jpeg_dc_kernel(const EDesc *__restrict__ descs, int16_t *__restrict__ coef) {
    __shared__ int sv[LANES];
    __shared__ int sf[LANES];
    const EDesc &e = descs[blockIdx.y];
    const int c = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (c >= e.ncomp || e.nlanes == 0) return;
    const int ch = e.ch[c], cv = e.cv[c], cbw = e.cbw[c], cblk0 = e.cblk0[c], mcux = e.mcux, interval = e.interval;
    const int hv = ch * cv, total = e.nmcu * hv, blocks = e.blocks;
    int16_t *base = coef + e.coef_base * 64;
    int carry = 0;
    for (int j0 = 0; j0 < total; j0 += LANES) {
        const int j = j0 + tid;
        int16_t *ptr = nullptr;
        int val = 0, flg = 0;
        if (j < total) {
            const int m = j / hv, w = j - m * hv, vv = w / ch, hh = w - vv * ch;
            const int my = m / mcux, mx = m - my * mcux;
            const int b = cblk0 + (my * cv + vv) * cbw + mx * ch + hh;
            if ((unsigned)b < (unsigned)blocks) {
                ptr = base + (int64_t)b * 64;
                val = ptr[0];
            }
            flg = (w == 0 && m % interval == 0) ? 1 : 0;
        }
        sv[tid] = val;
        sf[tid] = flg;
        __syncthreads();
        for (int d = 1; d < LANES; d <<= 1) {
            int tv = 0, tf = 0;
            if (tid >= d) {
                tv = sv[tid - d];
                tf = sf[tid - d];
            }
            __syncthreads();
            if (tid >= d && !sf[tid]) {
                sv[tid] += tv;
                sf[tid] = tf;
            }
            __syncthreads();
        }
        const int res = sv[tid] + (sf[tid] ? 0 : carry);
        if (ptr) ptr[0] = (int16_t)res;
        carry = sv[LANES - 1] + (sf[LANES - 1] ? 0 : carry);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void jpeg_clear_kernel(uint4 *__restrict__ p, int64_t n16) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0, 0, 0, 0);
}

// --------------------------------------------------------------------- host --
struct EntropyWork {
    int max_images = 0;
    int64_t max_blocks = 0;
    int gmax = 0;
    // pinned [flags × max_images | EDesc × max_images | GroupEnt × gmax] and its device twin
    PinBuf<uint8_t> h_meta;
    DevBuf<uint8_t> d_meta;
    size_t o_desc = 0, o_group = 0;
    PinBuf<int32_t> h_flags_out;  // pinned read-back
    DevBuf<uint8_t> d_ent;        // the uploaded segment tables and scans
    DevBuf<uint32_t> d_lexit, d_lcnt, d_group;  // d_group: gentry, gexit × 2, gtail
    std::vector<size_t> roff, rcap;  // each image's slice of the staging (begin): offset, bytes (0: not taken)
    size_t rtotal = 0;               // bytes of the staging the slices cover
    int32_t *h_flags() const { return reinterpret_cast<int32_t *>(h_meta.get()); }
    EDesc *h_desc() const { return reinterpret_cast<EDesc *>(h_meta.get() + o_desc); }
    GroupEnt *h_group() const { return reinterpret_cast<GroupEnt *>(h_meta.get() + o_group); }
};

EntropyWork *entropy_create(int max_images, int64_t max_blocks) {
    std::unique_ptr<EntropyWork> w(new EntropyWork());
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    w->max_images = max_images;
    w->max_blocks = max_blocks;
    w->gmax = (int)(max_blocks / LANES) + max_images;
    w->o_desc = al((size_t)max_images * 4);
    w->o_group = w->o_desc + al((size_t)max_images * sizeof(EDesc));
    const size_t meta = w->o_group + (size_t)w->gmax * sizeof(GroupEnt);
    w->h_meta.reserve(meta);
    w->d_meta.reserve(meta);
    w->h_flags_out.reserve((size_t)max_images);
    w->d_ent.reserve((size_t)max_blocks * 128);
    w->d_lexit.reserve((size_t)max_blocks);
    w->d_lcnt.reserve((size_t)max_blocks);
    w->d_group.reserve((size_t)w->gmax * 4);
    w->roff.assign(max_images, 0);
    w->rcap.assign(max_images, 0);
    return w.release();
}

void entropy_destroy(EntropyWork *w) { delete w; }

// Segments of the scan: restart intervals, or one.
static int64_t segment_count(const Header &hd) {
    const int64_t nmcu = (int64_t)hd.mcux * hd.mcuy;
    return hd.restart ? (nmcu + hd.restart - 1) / hd.restart : 1;
}

void entropy_begin(EntropyWork *w, int n, const Header *hd) {
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        w->h_flags()[i] = 1;  // until prepare takes the image
        w->h_desc()[i].nlanes = 0;
        // the slice: the segment table, every byte from SOS to the end of the data (stuffing and
        // markers only shrink it), each segment's padding to a dword, rounded to 128 B.  It is at
        // most the image's blocks × 128 B (else the host's), so the slices fit the staging.
        const int64_t nseg = segment_count(hd[i]);
        size_t need = (size_t)nseg * (sizeof(Seg) + 4) + (size_t)(hd[i].end - hd[i].scan) + 16;
        need = (need + 127) & ~(size_t)127;
        const bool fits = nseg > 0 && hd[i].blocks < ((int64_t)1 << 24) && need <= (size_t)hd[i].blocks * 128;
        w->roff[i] = off;
        w->rcap[i] = fits ? need : 0;
        off += w->rcap[i];
    }
    w->rtotal = off;
}

bool entropy_prepare(EntropyWork *w, int i, const Header &hd, int64_t blk_base, uint8_t *staging) {
    EDesc &e = w->h_desc()[i];
    std::memset(&e, 0, sizeof(e));
    const size_t cap = w->rcap[i];
    if (cap == 0) return false;  // scan above 128 B per block
    uint8_t *region = staging + w->roff[i];
    // the MCU's block slots, as decode_coefficients walks them
    int ns = 0;
    if (hd.ncomp == 1) {
        ns = 1;
    } else {
        for (int si = 0; si < hd.scan_ncomp; ++si) {
            const int ci = hd.scan_comp[si];
            const Comp &c = hd.c[ci];
            for (int v = 0; v < c.v; ++v)
                for (int h = 0; h < c.h; ++h) {
                    if (ns >= MAX_SLOTS) return false;
                    e.slot_comp[ns] = (uint8_t)ci;
                    e.slot_v[ns] = (uint8_t)v;
                    e.slot_h[ns] = (uint8_t)h;
                    ++ns;
                }
        }
    }
    const int64_t nmcu = (int64_t)hd.mcux * hd.mcuy;
    if (nmcu <= 0) return false;
    const int64_t interval = hd.restart ? hd.restart : nmcu;
    const int64_t nseg = segment_count(hd);
    if ((size_t)nseg * sizeof(Seg) + 8 > cap) return false;
    Seg *segs = reinterpret_cast<Seg *>(region);
    size_t wpos = (size_t)nseg * sizeof(Seg);
    const uint8_t *p = hd.scan, *end = hd.end;
    int64_t lanes = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const size_t start = wpos;
        int marker = -1;  // what ended the segment: a marker's second byte, or the data (-1)
        while (p < end) {
            const uint8_t *q = (const uint8_t *)std::memchr(p, 0xFF, (size_t)(end - p));
            const size_t run = (size_t)((q ? q : end) - p);
            if (wpos + run + 8 > cap) return false;  // more than 128 B per block: the host's
            std::memcpy(region + wpos, p, run);
            wpos += run;
            p += run;
            if (!q) break;
            if (q + 1 < end && q[1] == 0x00) {  // a stuffed 0xFF
                region[wpos++] = 0xFF;
                p = q + 2;
                continue;
            }
            marker = q + 1 < end ? q[1] : 0;  // p stays on the marker's 0xFF, as Bits::fill leaves it
            break;
        }
        // every segment but the last ends at its restart marker, numbered in order (Bits::restart)
        if (s + 1 < nseg) {
            if (marker != 0xD0 + (int)(s & 7)) return false;
            p += 2;
        }
        const size_t nbytes = wpos - start;
        while (wpos & 3) region[wpos++] = 0;
        for (size_t o = start; o < wpos; o += 4) {  // big-endian dwords: bit 0 of the stream is a dword's top bit
            uint32_t v;
            std::memcpy(&v, region + o, 4);
            v = __builtin_bswap32(v);
            std::memcpy(region + o, &v, 4);
        }
        segs[s].off = (uint32_t)start;
        segs[s].nbits = (uint32_t)(nbytes * 8);
        segs[s].lane0 = (uint32_t)lanes;
        segs[s].pad = 0;
        lanes += std::max<int64_t>(1, ((int64_t)nbytes * 8 + SUB_BITS - 1) / SUB_BITS);
    }
    if (lanes > hd.blocks) return false;  // the lanes' state words are sized by the blocks
    e.nlanes = (int32_t)lanes;
    e.nseg = (int32_t)nseg;
    e.nslots = ns;
    e.mcux = hd.mcux;
    e.nmcu = (int32_t)nmcu;
    e.interval = (int32_t)interval;
    e.lane_base = (int32_t)blk_base;
    e.ncomp = hd.ncomp;
    e.region_off = (int64_t)w->roff[i];
    e.coef_base = blk_base;
    e.blocks = (int32_t)hd.blocks;
    for (int c = 0; c < hd.ncomp; ++c) {
        e.ch[c] = hd.c[c].h;
        e.cv[c] = hd.c[c].v;
        e.cbw[c] = hd.c[c].bw;
        e.cblk0[c] = (int32_t)hd.c[c].blk0;
        const Huff *src[2] = {&hd.dc[hd.c[c].td], &hd.ac[hd.c[c].ta]};
        for (int t = 0; t < 2; ++t) {
            Tab &d = e.tab[2 * c + t];
            std::memcpy(d.look, src[t]->look, sizeof(d.look));
            std::memcpy(d.vals, src[t]->vals, sizeof(d.vals));
            for (int l = 10; l <= 16; ++l) {
                d.maxcode[l - 10] = src[t]->maxcode[l];
                d.delta[l - 10] = src[t]->delta[l];
            }
        }
    }
    w->h_flags()[i] = 0;
    return true;
}

size_t entropy_decode(EntropyWork *w, int n, int64_t nb, const uint8_t *staging, int16_t *d_coef, hipStream_t s,
                      int32_t *flags) {
    // the groups: LANES lanes of one image each
    GroupEnt *gr = w->h_group();
    int G = 0;
    bool chained = false;
    for (int i = 0; i < n; ++i) {
        const EDesc &e = w->h_desc()[i];
        if (e.nlanes == 0) continue;
        const Seg *segs = reinterpret_cast<const Seg *>(staging + e.region_off);
        const int g0 = G;
        int sg = 0;
        for (int l0 = 0; l0 < e.nlanes; l0 += LANES) {
            while (sg + 1 < e.nseg && segs[sg + 1].lane0 <= (uint32_t)l0) ++sg;
            GroupEnt &ge = gr[G++];
            ge.img = i;
            ge.lane0 = l0;
            ge.chained = segs[sg].lane0 != (uint32_t)l0;
            ge.gfirst = g0 + (int)(segs[sg].lane0 / LANES);
            chained = chained || ge.chained;
        }
    }
    size_t uploaded = w->o_desc + (size_t)n * sizeof(EDesc);
    RC_HIP(hipMemcpyAsync(w->d_meta.get(), w->h_meta.get(), uploaded, hipMemcpyHostToDevice, s));
    int32_t *d_flags = reinterpret_cast<int32_t *>(w->d_meta.get());
    if (G > 0) {
        RC_HIP(hipMemcpyAsync(w->d_meta.get() + w->o_group, gr, (size_t)G * sizeof(GroupEnt), hipMemcpyHostToDevice, s));
        // the scans: the images' slices lie back to back, one copy of about the files' bytes
        RC_HIP(hipMemcpyAsync(w->d_ent.get(), staging, w->rtotal, hipMemcpyHostToDevice, s));
        uploaded += (size_t)G * sizeof(GroupEnt) + w->rtotal;
        const EDesc *d_desc = reinterpret_cast<const EDesc *>(w->d_meta.get() + w->o_desc);
        const GroupEnt *d_gr = reinterpret_cast<const GroupEnt *>(w->d_meta.get() + w->o_group);
        uint32_t *gentry = w->d_group.get(), *gexit = w->d_group.get() + w->gmax, *gtail = w->d_group.get() + 3 * (size_t)w->gmax;
        const int64_t n16 = nb * 8;
        hipLaunchKernelGGL(jpeg_clear_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<uint4 *>(d_coef), n16);
        RC_LAUNCH_CHECK();
        const int passes = chained ? SYNC_PASSES : 1;
        for (int pass = 0; pass < passes; ++pass) {
            hipLaunchKernelGGL(jpeg_entropy_sync_kernel, dim3((unsigned)G), dim3(LANES), 0, s, d_desc, d_gr, w->d_ent.get(),
                               w->d_lexit.get(), w->d_lcnt.get(), gentry, gexit, gtail, w->gmax, pass);
            RC_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(jpeg_entropy_write_kernel, dim3((unsigned)G), dim3(LANES), 0, s, d_desc, d_gr, w->d_ent.get(),
                           w->d_lexit.get(), w->d_lcnt.get(), gentry, gexit + (size_t)((passes - 1) & 1) * w->gmax, gtail, d_coef, d_flags);
        RC_LAUNCH_CHECK();
        hipLaunchKernelGGL(jpeg_dc_kernel, dim3(3, (unsigned)n), dim3(LANES), 0, s, d_desc, d_coef);
        RC_LAUNCH_CHECK();
    }
    RC_HIP(hipMemcpyAsync(w->h_flags_out.get(), d_flags, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    RC_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) flags[i] = w->h_flags_out.get()[i];
    return uploaded;
}

}  // namespace jpeg
}  // namespace rc
