// svt-av1-1_amd/csrc/me_fullpel_common.h -- what the 85-PU (me_fullpel_impl.h) and the 209-PU (me_fullpel209_impl.h) full-pel search of
// one superblock by one 256-thread workgroup have in common: descriptor decode, window staging (general and, for the two-image form,
// fixed to a search width of 64), the raster lane -> item map, the
// square-PU key steps, the 8x8 class resolver, the per-item minima of the 85-PU class forms with their resolver and the 64x64 publish.  The row-step loops are NOT here: the three forms (one image
// pipelined, two images pipelined, 209-PU unpipelined with v_pk_mov_b32) differ for measured reasons.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "me_launch.h"
#include "me_sad_common.h"

// LDS row pitch of the staged reference window.  192 B: >= 16*8 + 64 (widest lane footprint at
// search_area_width 127) and == 48 dwords, which puts rows y, y+3, y+5, y+6 (one ds_read_b128 lane
// group) on four distinct bank quarters.
#define SVTHIP_FULLPEL_LDS_PITCH 192
// fixed LDS in front of the window: 16 KB exchange buffer + 64 B
#define SVTHIP_FULLPEL_LDS_FIXED (16384 + 64)

namespace svthip {

inline size_t fullpel_lds_bytes(uint32_t max_sh) { return SVTHIP_FULLPEL_LDS_FIXED + (size_t)(max_sh + 63) * SVTHIP_FULLPEL_LDS_PITCH; }

// me_fullpel209.hip: the 209-PU arm of launch_fullpel (me_fullpel.hip), same arguments
SVTHIP_LOCAL hipError_t launch_fullpel209(const uint8_t* src, uint32_t src_stride, const uint8_t* ref, uint32_t ref_stride,
                                          const svthip_fullpel_desc* desc, uint32_t n_sb, uint32_t max_sh, uint32_t* out_sad, uint32_t* out_mv,
                                          hipStream_t s);

constexpr int kPitch = SVTHIP_FULLPEL_LDS_PITCH;  // bytes per window row in LDS (one-image plans)

// a superblock's descriptor (6 int32: src_offset, ref_offset, x/y search origin, search width/height) and what follows from it:
// column groups of 16 positions per search row, and 2^16 / n_xg rounded up for the division by n_xg
struct FullpelDesc {
    int src_off, ref_off, xo, yo, sw, sh, n_xg;
    uint32_t inv_xg;
};

// d: any address space.  The values are wave-uniform by construction; readfirstlane keeps them in SGPRs also when the descriptor is
// read from LDS
__device__ __forceinline__ FullpelDesc fullpel_decode_desc(const int32_t* d)
{
    FullpelDesc D;
    D.src_off = __builtin_amdgcn_readfirstlane(d[0]);
    D.ref_off = __builtin_amdgcn_readfirstlane(d[1]);
    D.xo = __builtin_amdgcn_readfirstlane(d[2]);
    D.yo = __builtin_amdgcn_readfirstlane(d[3]);
    D.sw = __builtin_amdgcn_readfirstlane(d[4]);
    D.sh = __builtin_amdgcn_readfirstlane(d[5]);
    D.n_xg = (D.sw + 15) >> 4;
    D.inv_xg = (65536u + (uint32_t)D.n_xg - 1u) / (uint32_t)D.n_xg;  // wave-uniform, scalar unit
    return D;
}

// Stages the reference window at `base` into LDS at `win`, PITCH bytes per row: rows 0..sh+62, bytes 0..sw+62 valid, zero beyond.
// 16 bytes per thread and pass, read at the window's own byte alignment (global loads need no alignment on this target) and written as
// one ds_write_b128: 6 passes for a 64x64 area instead of 24 dword passes with a second load + v_alignbyte each.
// IMAGE1 != 0 (the two-image LDS plan, me_fullpel_img2.h): a second image IMAGE1 bytes behind the first holds the same window one
// dword later (the same bytes of the plane, so nothing new is read).
template <int PITCH, int IMAGE1 = 0>
__device__ __forceinline__ void stage_window(uint8_t* win, const uint8_t* base, uint32_t ref_stride, int sw, int sh, int tid)
{
    const int rows = sh + 63;
    const int ndw_valid = (sw + 63 + 3) >> 2;
    constexpr int q_row = PITCH >> 4;
    const int total = rows * q_row;
    // one 16-byte slot of a window row; left = dwords of it that belong to the window
    auto slot = [](const uint8_t* p, int left) {
        uint32_t t[4] = {0u, 0u, 0u, 0u};
        if (left >= 4) {
            const unaligned_u32x4 u = *reinterpret_cast<const unaligned_u32x4*>(p);
            t[0] = u.v[0]; t[1] = u.v[1]; t[2] = u.v[2]; t[3] = u.v[3];
        } else if (left > 0) {  // the row's last dwords: nothing is read past them
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (k < left) t[k] = reinterpret_cast<const unaligned_u32*>(p + 4 * k)->v;
        }
        return make_uint4(t[0], t[1], t[2], t[3]);
    };
    for (int i = tid; i < total; i += 256) {
        const int r = i / q_row;
        const int c4 = i - r * q_row;
        const uint8_t* p = base + (size_t)r * ref_stride + 16 * c4;
        const int left = ndw_valid - 4 * c4;
        reinterpret_cast<uint4*>(win)[i] = slot(p, left);
        if constexpr (IMAGE1 != 0) reinterpret_cast<uint4*>(win + IMAGE1)[i] = slot(p + 4, left - 1);
    }
}

// The same for the two-image form, which runs only at sw == 64 (me_fullpel.hip): a window row has 32 dwords, so image 0 takes eight full
// 16-byte slots, image 1 dwords 1..32 of which the last is past the window and stays zero, and slot 8 of both images is zero.  The LDS
// contents equal stage_window<PITCH, IMAGE1>(win, base, ref_stride, 64, sh, tid)'s byte for byte and no other byte of the plane is read.
// Thread -> (row = tid >> 3, + 32 per pass, slot = tid & 7), MAX_PASSES unrolled passes (sh + 63 <= 32 * MAX_PASSES): no division, and
// the row pointer advances by an add.  Image 1's slot is dwords 1..3 of the thread's own image-0 slot and ONE more dword (none in
// slot 7), not a second 16-byte load.
template <int PITCH, int IMAGE1, int MAX_PASSES>
__device__ __forceinline__ void stage_window64(uint8_t* win, const uint8_t* base, uint32_t ref_stride, int sh, int tid)
{
    static_assert(PITCH == 144 && IMAGE1 != 0, "nine 16-byte slots per row, two images");
    const int rows = sh + 63;
    const int c4 = tid & 7;
    const int r0 = tid >> 3;
    const uint8_t* p = base + (size_t)r0 * ref_stride + 16 * c4;
    uint8_t* w = win + r0 * PITCH + 16 * c4;
    // every pass's loads go out before the first LDS write waits for one
    unaligned_u32x4 u[MAX_PASSES];
    uint32_t next[MAX_PASSES];
#pragma unroll
    for (int k = 0; k < MAX_PASSES; k++, p += 32 * (size_t)ref_stride) {
        u[k] = unaligned_u32x4{{0u, 0u, 0u, 0u}};
        next[k] = 0u;
        if (r0 + 32 * k < rows) {
            u[k] = *reinterpret_cast<const unaligned_u32x4*>(p);
            if (c4 < 7) next[k] = reinterpret_cast<const unaligned_u32*>(p + 16)->v;
        }
    }
#pragma unroll
    for (int k = 0; k < MAX_PASSES; k++) {
        if (r0 + 32 * k < rows) {
            *reinterpret_cast<uint4*>(w + 32 * k * PITCH) = make_uint4(u[k].v[0], u[k].v[1], u[k].v[2], u[k].v[3]);
            *reinterpret_cast<uint4*>(w + 32 * k * PITCH + IMAGE1) = make_uint4(u[k].v[1], u[k].v[2], u[k].v[3], next[k]);
        }
    }
    if (tid < 2 * rows) *reinterpret_cast<uint4*>(win + (tid & 1) * IMAGE1 + (tid >> 1) * PITCH + 128) = make_uint4(0u, 0u, 0u, 0u);
}

// Raster map of search iteration `it`: lane l holds item 64 it + l, an item being 16 horizontally consecutive positions (column group
// xg of search row y).  A lane past the last item repeats item 0: its keys duplicate a first-pass lane's and change no minimum
// (whatever is not a plain minimum checks the returned lane_valid).
__device__ __forceinline__ bool fullpel_raster_item(int it, int lane, int n_items, int n_xg, uint32_t inv_xg, int& y, int& xg)
{
    int pg = it * 64 + lane;
    const bool lane_valid = pg < n_items;
    if (!lane_valid) pg = 0;
    y = (int)(((uint32_t)pg * inv_xg) >> 16);  // pg / n_xg, exact for n_xg <= 8 and pg < 1024 (the emulated division is ~20 instructions)
    xg = pg - y * n_xg;
    return lane_valid;
}
// raster index (y * 128 + x) of an item's first position
__device__ __forceinline__ uint32_t fullpel_idx0(int y, int xg) { return (uint32_t)(y * 128 + 16 * xg); }

// 8x8 PUs per position CLASS: the four quads of a lane's 16 positions (acc[q]: packed u16 SADs of positions 4 q .. 4 q + 3) are first
// reduced with packed 16-bit minima (slot c of the result = min over q of the SAD at position 4 q + c), then ONE quad of keys
// (sad << 16 | idx[c]) goes into the running minimum: 12 instructions per PU and item instead of 24.  resolve_class8 finds the position.
__device__ __forceinline__ uint32_t track_class8(uint32_t best, const uint64_t (&acc)[4], const uint32_t* idx, uint32_t himask)
{
    const uint32_t mlo = pk_min_u16(pk_min_u16((uint32_t)acc[0], (uint32_t)acc[1]), pk_min_u16((uint32_t)acc[2], (uint32_t)acc[3]));
    const uint32_t mhi = pk_min_u16(pk_min_u16((uint32_t)(acc[0] >> 32), (uint32_t)(acc[1] >> 32)),
                                    pk_min_u16((uint32_t)(acc[2] >> 32), (uint32_t)(acc[3] >> 32)));
    return track4(best, pack64(mlo, mhi), idx, himask);
}

// 32x32 = sum of the four 16x16 ([zz][q] packed u16 sums): pairs are added packed (<= 2*32640 fits u16), then widened
__device__ __forceinline__ void widen_sums32(const uint32_t (&s16lo)[4][4], const uint32_t (&s16hi)[4][4], uint32_t (&s32acc)[16])
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t a_lo = s16lo[0][q] + s16lo[1][q], b_lo = s16lo[2][q] + s16lo[3][q];
        const uint32_t a_hi = s16hi[0][q] + s16hi[1][q], b_hi = s16hi[2][q] + s16hi[3][q];
        s32acc[4 * q + 0] = (a_lo & 0xffffu) + (b_lo & 0xffffu);
        s32acc[4 * q + 1] = (a_lo >> 16) + (b_lo >> 16);
        s32acc[4 * q + 2] = (a_hi & 0xffffu) + (b_hi & 0xffffu);
        s32acc[4 * q + 3] = (a_hi >> 16) + (b_hi >> 16);
    }
}

// 32x32 PU of a quadrant: key = raw << 14 | idx  (raw <= 130560 < 2^17)
__device__ __forceinline__ uint32_t track32(uint32_t best, const uint32_t (&s32acc)[16], const uint32_t (&idx)[16])
{
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        uint32_t k0 = (s32acc[i] << 14) | idx[i];
        uint32_t k1 = (s32acc[i + 1] << 14) | idx[i + 1];
        best = min3u(best, k0, k1);
    }
    return best;
}

// ---- per-ITEM minima (the class forms of the 85-PU search) ----
// A lane visits only a few items per PU, an item being a run of 16 consecutive raster positions, and items are disjoint.  So the first
// minimum in raster order is in the first item that attains the minimum SAD, and inside that item it is the first position that attains
// it.  The search loop tracks the first part alone: key = (minimum SAD of the item) << k | idx0, idx0 = the item's first raster index
// (fullpel_idx0; its low four bits are free).  resolve_items recomputes the second part after the search, once per superblock.

// packed u16 SADs or sums of an item's 16 positions (8 dwords): 7 v_pk_min_u16 leave the minimum over the even positions in the low
// half and over the odd ones in the high half; two keys, one v_min3 -- 10 instructions per PU and item
__device__ __forceinline__ uint32_t track_item16(uint32_t best, const uint32_t (&d)[8], uint32_t idx0, uint32_t himask)
{
    const uint32_t m = pk_min_u16_tree(pk_min_u16_tree(pk_min_u16_tree(d[0], d[1]), pk_min_u16_tree(d[2], d[3])),
                                       pk_min_u16_tree(pk_min_u16_tree(d[4], d[5]), pk_min_u16_tree(d[6], d[7])));
    return min3u(best, (m << 16) | idx0, (m & himask) | idx0);
}

// The 8x8 PUs reduce an item in four instructions instead of seven.  A raw 8x8 SAD (32 pixels) is at most 32 * 255 = 8160 = 0x1fe0, and
// every u16 below 0x7c00 is the bit pattern of a non-negative finite f16 whose order is the integer order, so v_pk_minimum3_f16 is an
// exact three-input packed u16 minimum on such values (1..1023 are denormals: the kernels run with f16 denormals on, the default,
// and a minimum returns one of its operands unchanged).  The 16x16 sums reach 4 * 8160 = 0x7f80 >= 0x7c00 (infinity and NaN patterns)
// and keep track_item16.  Never feed it anything but raw 8x8 SADs: 0xffff, the trackers' initial value, is a NaN.
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_min3_f16bits(uint32_t a, uint32_t b, uint32_t c)
{
    const f16x2_t x = __builtin_bit_cast(f16x2_t, a), y = __builtin_bit_cast(f16x2_t, b), z = __builtin_bit_cast(f16x2_t, c);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_minimum(__builtin_elementwise_minimum(x, y), z));
}
// packed u16 raw 8x8 SADs of an item's 16 positions: the minimum over the even positions in the low half, over the odd ones in the high half
__device__ __forceinline__ uint32_t item_min8(const uint32_t (&d)[8])
{
    return pk_min_u16_tree(pk_min3_f16bits(d[0], d[1], d[2]), pk_min3_f16bits(pk_min3_f16bits(d[3], d[4], d[5]), d[6], d[7]));
}
// one-image class form: key per pass as in track_item16 -- 7 instructions per PU and item
__device__ __forceinline__ uint32_t track_item8(uint32_t best, const uint32_t (&d)[8], uint32_t idx0, uint32_t himask)
{
    const uint32_t m = item_min8(d);
    return min3u(best, (m << 16) | idx0, (m & himask) | idx0);
}
// Two-image class form: a lane's items are search rows 16 it + lane_row, it = 0..3, so among a lane's OWN items the raster order is the
// order of `it`, and 4 * 8160 + 3 = 0x7f83 fits 16 bits: the running value is the packed u16 minimum of 4 * sad + it (run starts at
// 0xffffffff, tag = it * 0x00010001; m << 2 cannot carry between the halves because m.lo <= 0x1fe0) -- 6 instructions per PU and item.
// item_key8 turns it, once per superblock, into the key that track_item16 would have left: the lane's minimum SAD with the first raster
// index (idx0) of the first of its items that attains it.
__device__ __forceinline__ uint32_t track_item8_tagged(uint32_t run, const uint32_t (&d)[8], uint32_t tag)
{
    return pk_min_u16_tree(run, (item_min8(d) << 2) | tag);
}
// lane_idx0: fullpel_idx0(lane_row, column group), the lane's item of pass 0 (below 2048; a pass adds 16 rows = 2048)
__device__ __forceinline__ uint32_t item_key8(uint32_t run, uint32_t lane_idx0)
{
    const uint32_t r = min(run & 0xffffu, run >> 16);
    return ((r >> 2) << 16) | ((r & 3u) << 11) | lane_idx0;
}

// 32x32 PU of a quadrant: the 16 widened sums of an item (raw <= 130560 < 2^17), key = min << 14 | idx0 -- 7 v_min3, two keys, one v_min3
__device__ __forceinline__ uint32_t track_item32(uint32_t best, const uint32_t (&s32acc)[16], uint32_t idx0)
{
    uint32_t m = min3u(s32acc[0], s32acc[1], s32acc[2]);
#pragma unroll
    for (int i = 3; i < 15; i += 2) m = min3u(m, s32acc[i], s32acc[i + 1]);
    return min3u(best, (m << 14) | idx0, (s32acc[15] << 14) | idx0);
}

// 64x64 PU of areas up to 64x64: the sum is below 2^19 and y * 64 + x below 2^12, so (sum << 12 | y * 64 + x) is a 32-bit key that keeps
// the raster order.  sv: the sums at positions (y, x0 .. x0 + 3).  Every lane's item lies inside the area (a lane without an item of its
// own repeats another lane's), so no key needs masking.
__device__ __forceinline__ uint32_t track_quad64(uint32_t best, const uint32_t (&sv)[4], int y, int x0)
{
    const uint32_t i0 = (uint32_t)(y * 64 + x0);
    best = min3u(best, (sv[0] << 12) | i0, (sv[1] << 12) | (i0 + 1u));
    return min3u(best, (sv[2] << 12) | (i0 + 2u), (sv[3] << 12) | (i0 + 3u));
}

// origin, inside its 32x32 quadrant, of 8x8 PU p = 4 zz + k (16x16 block zz, 8x8 k of it: the order of the 8x8 trackers)
__device__ __forceinline__ void pu8_origin(int p, int& px, int& py)
{
    const int zz = p >> 2, k = p & 3;
    px = 16 * (zz & 1) + 8 * (k & 1);
    py = 16 * (zz >> 1) + 8 * (k >> 1);
}

// Resolves the 8x8 winners of quadrant Q after the class search.  The winner of a PU names its item and its SAD
// (key = sad << 16 | y * 128 + 16 * xg + class) but not the position inside the item: items are disjoint runs of 16 raster positions, so
// the first minimum in raster order lies in the first item that attains the minimum -- which is what the key order picks.  Lane =
// 4 * PU + quad recomputes the SADs of positions 4 quad .. 4 quad + 3 of that item (8 v_qsad per lane, once per superblock) from the
// PU's eight source dwords rs (rows 0, 2, 4, 6 at pu8_origin), and the first position whose SAD equals the minimum is the reference's strict-'<' winner.
// key: the winning key of PU lane >> 2.
template <int PITCH>
__device__ __forceinline__ void resolve_class8(const uint8_t* win, uint32_t key, const uint32_t (&rs)[4][2], int lane, int Q, int xo, int yo,
                                               uint32_t* osad, uint32_t* omv)
{
    const int p = lane >> 2, q = lane & 3;
    const uint32_t s = key >> 16, id = key & 0xffffu;
    const int y = (int)(id >> 7), xb = (int)(id & 0x70u);
    int px, py;
    pu8_origin(p, px, py);
    const uint8_t* wp = win + (y + 32 * (Q >> 1) + py) * PITCH + xb + 4 * q + 32 * (Q & 1) + px;
    uint64_t a = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(wp + 2 * r * PITCH);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
        a = __builtin_amdgcn_qsad_pk_u16_u8(pack64(w0, w1), rs[r][0], a);
        a = __builtin_amdgcn_qsad_pk_u16_u8(pack64(w1, w2), rs[r][1], a);
    }
    const uint32_t lo = (uint32_t)a, hi = (uint32_t)(a >> 32);
    uint32_t first = (lo & 0xffffu) == s ? 0u : (lo >> 16) == s ? 1u : (hi & 0xffffu) == s ? 2u : (hi >> 16) == s ? 3u : 64u;
    first += 4u * (uint32_t)q;
    first = min(first, (uint32_t)__shfl_xor((int)first, 1));
    first = min(first, (uint32_t)__shfl_xor((int)first, 2));
    if (q == 0) {
        const int pu = 21 + 16 * Q + p;
        osad[pu] = 2u * s;
        omv[pu] = mv_word(xo + xb + (int)first, yo + y);
    }
}

// Resolves the 8x8, 16x16 and 32x32 winners of quadrant Q after the per-item search (track_item16 / track_item32) in three passes over
// the same lanes: lane = 4 * part + quad, part = one of the quadrant's sixteen 8x8 blocks (order of pu8_origin), recomputes the part's
// SADs at positions 4 quad .. 4 quad + 3 of an item from the part's eight source dwords rs (8 v_qsad per lane and pass).
//   pass 0: every part at the item of its own 8x8 winner (key8, SAD in key >> 16);
//   pass 1: every part at the item of its 16x16 PU's winner (key16): the four part lanes of a PU and quad are added, packed u16;
//   pass 2: every part at the item of the 32x32 winner (key32, SAD in key >> 14): all sixteen part lanes are added, packed while the
//           sums fit 16 bits (8 parts: <= 65280), widened for the last step.
// The first position whose recomputed SAD equals the tracked minimum is the reference's strict-'<' winner.
template <int PITCH>
__device__ __forceinline__ void resolve_items(const uint8_t* win, uint32_t key8, uint32_t key16, uint32_t key32, const uint32_t (&rs)[4][2],
                                              int lane, int Q, int xo, int yo, uint32_t* osad, uint32_t* omv)
{
    const int p = lane >> 2, q = lane & 3;
    int px, py;
    pu8_origin(p, px, py);
    const uint8_t* wpart = win + (32 * (Q >> 1) + py) * PITCH + 4 * q + 32 * (Q & 1) + px;
#pragma unroll
    for (int pass = 0; pass < 3; pass++) {
        const uint32_t key = pass == 0 ? key8 : pass == 1 ? key16 : key32;
        const int kbits = pass == 2 ? 14 : 16;
        const uint32_t s = key >> kbits, id = key & ((1u << kbits) - 1u);
        const int y = (int)(id >> 7), xb = (int)(id & 0x70u);
        const uint8_t* wp = wpart + y * PITCH + xb;
        uint64_t a = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(wp + 2 * r * PITCH);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
            a = __builtin_amdgcn_qsad_pk_u16_u8(pack64(w0, w1), rs[r][0], a);
            a = __builtin_amdgcn_qsad_pk_u16_u8(pack64(w1, w2), rs[r][1], a);
        }
        uint32_t lo = (uint32_t)a, hi = (uint32_t)(a >> 32);
        if (pass >= 1) {  // the four parts of a 16x16: lanes ^ 4, ^ 8
            lo += (uint32_t)__shfl_xor((int)lo, 4); hi += (uint32_t)__shfl_xor((int)hi, 4);
            lo += (uint32_t)__shfl_xor((int)lo, 8); hi += (uint32_t)__shfl_xor((int)hi, 8);
        }
        if (pass == 2) {  // two 16x16 still packed
            lo += (uint32_t)__shfl_xor((int)lo, 16); hi += (uint32_t)__shfl_xor((int)hi, 16);
        }
        uint32_t c[4] = {lo & 0xffffu, lo >> 16, hi & 0xffffu, hi >> 16};
        if (pass == 2) {
#pragma unroll
            for (int j = 0; j < 4; j++) c[j] += (uint32_t)__shfl_xor((int)c[j], 32);
        }
        uint32_t first = c[0] == s ? 0u : c[1] == s ? 1u : c[2] == s ? 2u : c[3] == s ? 3u : 64u;
        first += 4u * (uint32_t)q;
        first = min(first, (uint32_t)__shfl_xor((int)first, 1));
        first = min(first, (uint32_t)__shfl_xor((int)first, 2));
        const int pu_lanes = pass == 0 ? 4 : pass == 1 ? 16 : 64;
        if ((lane & (pu_lanes - 1)) == 0) {
            const int pu = pass == 0 ? 21 + 16 * Q + p : pass == 1 ? 5 + 4 * Q + (p >> 2) : 1 + Q;
            osad[pu] = 2u * s;
            omv[pu] = mv_word(xo + xb + (int)first, yo + y);
        }
    }
}

// a PU's result from its raw SAD and the raster index of its best position (idx = y * 128 + x, 14 bits)
__device__ __forceinline__ void store_pu(uint32_t* osad, uint32_t* omv, int pu, uint32_t raw, uint32_t id, int xo, int yo)
{
    osad[pu] = 2u * raw;
    omv[pu] = mv_word(xo + (int)(id & 127u), yo + (int)(id >> 7));
}

// 64x64 PU: a wave's lanes hold (raw SAD, raster index) of their best position; the four waves meet in the 64-bit LDS cell (set to ~0
// while the window is staged), which holds the superblock's (raw << 32 | idx) after the next barrier (read_best64)
__device__ __forceinline__ void merge_best64(unsigned long long* best64_lds, uint32_t raw, uint32_t idx, int lane)
{
    const unsigned long long k64 = wave_min_u64(((unsigned long long)raw << 32) | idx);
    if (lane == 0) atomicMin(best64_lds, k64);
}
__device__ __forceinline__ void read_best64(const unsigned long long* best64_lds, uint32_t& raw, uint32_t& id)
{
    const unsigned long long k = *best64_lds;
    raw = (uint32_t)(k >> 32);
    id = (uint32_t)k;
}
// the same for lanes that hold a 32-bit key of track_quad64: the cell's low dword carries the key
__device__ __forceinline__ void merge_best64_key(unsigned long long* best64_lds, uint32_t key, int lane)
{
    const uint32_t k = wave_min_u32(key);
    if (lane == 0) atomicMin(reinterpret_cast<uint32_t*>(best64_lds), k);
}
__device__ __forceinline__ void read_best64_key(const unsigned long long* best64_lds, uint32_t& raw, uint32_t& id)
{
    const uint32_t k = *reinterpret_cast<const uint32_t*>(best64_lds);
    raw = k >> 12;
    id = ((k & 0xfc0u) << 1) | (k & 63u);  // y * 64 + x -> y * 128 + x
}

}  // namespace svthip
