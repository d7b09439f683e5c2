// svt-av1-1_amd/csrc/me_hme_impl.h -- search-centre derivation of one superblock by one 256-thread workgroup (device code).
// Included inside namespace svthip { namespace { ... } } by me_hme.hip, which includes me_sad_common.h (pack64, min3u, wave_min_u32 / _u64,
// u32x4_t, unaligned_u32x4) first.  (A kernel fusing this chain with the full-pel search of the same superblock was bit-identical but
// slower -- both halves are VALU-bound -- and was removed.)  See me_hme.hip for the mapping and the reference citations.
// Which search loop a level of a superblock takes is decided in hme_level0_search and hme_level_search alone; the header comment of each
// loop names the shapes that reach it.  The LDS loops read the source block that the workgroup staged (HmeShared::src0 / 1 / 2).
#pragma once


// Unaligned 4-byte read as two ALIGNED dword loads + v_alignbyte.  A single misaligned global_load_dword is
// legal on gfx950; round 1 measured it ~10x slower in the un-staged search loop (the 64 lanes of a wave split into per-lane
// requests), while for the staging copies (stage_window_rows, the full-pel and sub-pel windows) byte-aligned dword / dwordx4
// loads turned out as fast as aligned ones and are used there.  The centre check keeps this form (no measurable difference).
// The aligned address is rebuilt from an integer; the pointer type carries the GLOBAL address space explicitly, otherwise the
// integer-to-pointer cast yields a generic pointer and every load becomes a flat_load (which also ties the loads to the LDS
// counter).  Everything these helpers read lives in the picture pool.
typedef const __attribute__((address_space(1))) uint32_t gmem_u32;
typedef const __attribute__((address_space(1))) unaligned_u32x4 gmem_u32x4;  // 16 bytes at byte alignment: one global_load_dwordx4

__device__ __forceinline__ uint32_t ldu32(const uint8_t* p)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    gmem_u32* q = (gmem_u32*)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3u);
    const uint32_t lo = q[0];
    const uint32_t hi = sh ? q[1] : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
}

// branch-free variant for bulk copies: always reads both aligned dwords (up to 7 bytes past p: pool slack)
__device__ __forceinline__ uint32_t ldu32_nb(const uint8_t* p)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    gmem_u32* q = (gmem_u32*)(a & ~(uintptr_t)3);
    return __builtin_amdgcn_alignbyte(q[1], q[0], (uint32_t)(a & 3u));
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// Optional per-phase time stamps (tools/hme_stamps_probe.py builds a copy of the library with -DSVTHIP_HME_STAMPS): s_memtime of lane 0 of
// every region wave at the phase boundaries of hme_center_sb, [superblock][wave][8].
// Wave priority around the latency-bound pieces (source staging, centre checks, window copies); -DSVTHIP_HME_NO_PRIO for A/B timing.
#ifdef SVTHIP_HME_NO_PRIO
#define HME_PRIO(p) do { } while (0)
#else
#define HME_PRIO(p) __builtin_amdgcn_s_setprio(p)
#endif
#ifdef SVTHIP_HME_STAMPS
__device__ unsigned long long g_hme_stamps[8192 * 4 * 8];
#define HME_STAMP(i)                                                                                                          \
    do {                                                                                                                      \
        if (lane == 0 && sbi < 8192u) g_hme_stamps[((size_t)sbi * 4 + (threadIdx.x >> 6)) * 8 + (i)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
// sub-phases of wave_sad_loop_lds, summed over all waves of the launches since load: [W == 64][staging, search loop, tail, calls]
__device__ unsigned long long g_hme_loop_phase[2 * 4];
#define HME_LOOP_T(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define HME_LOOP_ADD(slot, t1, t0)                                                                                \
    do {                                                                                                          \
        if (lane == 0) atomicAdd(&g_hme_loop_phase[(W == 64 ? 4 : 0) + (slot)], (unsigned long long)((t1) - (t0))); \
    } while (0)
#else
#define HME_STAMP(i) do { } while (0)
#define HME_LOOP_T(var) do { } while (0)
#define HME_LOOP_ADD(slot, t1, t0) do { } while (0)
#endif

// Per-wave LDS slice: a band of the search window (the source blocks of full SBs sit in HmeShared).  7 KB holds the whole level-0 window
// of the 1080p 200 % area (96 x 48 positions: 62 rows x 28 dwords = 6 944 B) in one band; 4 slices + HmeShared stay under
// 32 KB per workgroup, five workgroups per CU.
constexpr int kHmeLdsPerWave = 7 * 1024;

// The 64 x 32-row reference block of a centre check (stride already doubled) in two halves, so that a caller can issue the loads
// before the barrier that publishes the staged source block: lane = (row mod 4, dword column), eight rows per lane.
__device__ __forceinline__ void load_ref_block64(const uint8_t* ref, uint32_t ref_stride, int lane, uint32_t (&tv)[8])
{
    const uint32_t c = (uint32_t)lane & 15u, r0 = (uint32_t)lane >> 4;
    const uint8_t* rp = ref + (size_t)r0 * ref_stride + 4u * c;
#pragma unroll
    for (int k = 0; k < 8; k++) tv[k] = ldu32_nb(rp + (size_t)(4 * k) * ref_stride);
}

__device__ __forceinline__ uint32_t sad_ref_block64(const uint32_t (&tv)[8], const uint32_t* src_lds, int lane)
{
    const uint32_t c = (uint32_t)lane & 15u, r0 = (uint32_t)lane >> 4;
    uint32_t acc4 = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) acc4 = __builtin_amdgcn_sad_u8(src_lds[(r0 + 4 * k) * 16 + c], tv[k], acc4);
    return wave_sum_u32(acc4);
}

// SAD of a W x H block (strides already doubled by the caller), computed by one wave.  W need not be a
// multiple of 4: the tail dword is masked on both operands.
__device__ uint32_t wave_block_sad(const uint8_t* src, uint32_t src_stride, const uint8_t* ref, uint32_t ref_stride,
                                   uint32_t H, uint32_t W, int lane, const uint32_t* src_lds = nullptr)
{
    if (src_lds && W == 64 && H == 32) {
        // the 64 x 32-row source block is already in LDS ([32][16] dwords): only the reference rows come from memory
        uint32_t tv[8];
        load_ref_block64(ref, ref_stride, lane, tv);
        return sad_ref_block64(tv, src_lds, lane);
    }
    if (W == 64 && (H & 3u) == 0) {
        // full-width block: lane = (row mod 4, dword column), four rows per pass, all loads of a lane in flight together;
        // src is dword aligned (SB origin multiple of 64), ref is re-aligned from aligned pairs
        const uint32_t c = (uint32_t)lane & 15u, r0 = (uint32_t)lane >> 4;
        const uint8_t* sp = src + (size_t)r0 * src_stride + 4u * c;
        const uint8_t* rp = ref + (size_t)r0 * ref_stride + 4u * c;
        uint32_t acc4 = 0;
        for (uint32_t r = 0; r < H; r += 16) {
            uint32_t sv[4], tv[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const bool in = r + 4u * (uint32_t)k < H;  // uniform
                sv[k] = in ? *reinterpret_cast<const uint32_t*>(sp + (size_t)(4 * k) * src_stride) : 0u;
                tv[k] = in ? ldu32_nb(rp + (size_t)(4 * k) * ref_stride) : 0u;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) acc4 = __builtin_amdgcn_sad_u8(sv[k], tv[k], acc4);
            sp += (size_t)16 * src_stride;
            rp += (size_t)16 * ref_stride;
        }
        return wave_sum_u32(acc4);
    }
    const uint32_t ndw = (W + 3) >> 2;
    const uint32_t n = H * ndw;
    uint32_t acc = 0;
    for (uint32_t i = lane; i < n; i += 64) {
        const uint32_t r = i / ndw, c = i - r * ndw;
        uint32_t s = ldu32(src + (size_t)r * src_stride + 4 * c);
        uint32_t t = ldu32(ref + (size_t)r * ref_stride + 4 * c);
        const uint32_t rem = W - 4 * c;
        if (rem < 4) {
            const uint32_t m = (1u << (8 * rem)) - 1u;
            s &= m;
            t &= m;
        }
        acc = __builtin_amdgcn_sad_u8(s, t, acc);
    }
    return wave_sum_u32(acc);
}

// The tail of every search loop.  The best key is made wave-uniform first, so that the decode, and the origin arithmetic, window clipping
// and loop bounds of the next level, are scalar code instead of vector code under exec masks.
__device__ __forceinline__ void store_best(uint32_t sad, uint32_t pos, uint32_t sw, uint32_t* best_sad, int* bx, int* by)
{
    *best_sad = sad;
    *by = (int)(pos / sw);
    *bx = (int)(pos - (uint32_t)(*by) * sw);
}

// key = sad << pos_bits | raster index
__device__ __forceinline__ void wave_best_u32(uint32_t key, int pos_bits, int sw, uint32_t* best_sad, int* bx, int* by)
{
    key = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_min_u32(key));
    store_best(key >> pos_bits, key & ((1u << pos_bits) - 1u), (uint32_t)sw, best_sad, bx, by);
}

// key = sad << 32 | raster index
__device__ __forceinline__ void wave_best_u64(unsigned long long key, int sw, uint32_t* best_sad, int* bx, int* by)
{
    key = wave_min_u64(key);
    store_best((uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(key >> 32)), (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)key),
               (uint32_t)sw, best_sad, bx, by);
}

// Generic SadLoopKernel by one wave straight from global memory (any block shape): partial SBs, and full SBs whose window rows are so wide
// that no band fits the LDS slice (hme_bands).
__device__ void wave_sad_loop_generic(const uint8_t* src, uint32_t src_stride, const uint8_t* ref, uint32_t ref_stride,
                                      uint32_t H, uint32_t W, uint32_t ref_stride_raw, int sw, int sh, int lane,
                                      uint32_t* best_sad, int* bx, int* by)
{
    const int npos = sw * sh;
    unsigned long long best = ~0ull;
    const uint32_t ndw = (W + 3) >> 2;
    const uint32_t tail = W & 3u;
    const uint32_t tailmask = tail ? ((1u << (8 * tail)) - 1u) : 0xffffffffu;
#pragma unroll 1
    for (int pos = lane; pos < npos; pos += 64) {
        const int y = pos / sw, x = pos - y * sw;
        const uint8_t* r0 = ref + (size_t)y * ref_stride_raw + x;
        uint32_t acc = 0;
#pragma unroll 1
        for (uint32_t r = 0; r < H; r++) {
            const uint8_t* sp = src + (size_t)r * src_stride;
            const uint8_t* rp = r0 + (size_t)r * ref_stride;
#pragma unroll 2
            for (uint32_t c = 0; c < ndw; c++) {
                uint32_t s = ldu32(sp + 4 * c);
                uint32_t t = ldu32(rp + 4 * c);
                if (c == ndw - 1) {
                    s &= tailmask;
                    t &= tailmask;
                }
                acc = __builtin_amdgcn_sad_u8(s, t, acc);
            }
        }
        const unsigned long long key = ((unsigned long long)acc << 32) | (uint32_t)pos;
        best = key < best ? key : best;  // a lane visits its positions in raster order
    }
    wave_best_u64(best, sw, best_sad, bx, by);
}

// Copies `wrows` plane rows of `pitch` dwords each, starting at the (unaligned) address `base`, into LDS (row r at win + r * pitch).
// Reads up to pitch * 4 + 19 bytes per row (the pool's tail slack covers the last row of the last plane).  pitch <= 256 (a band of at
// least 15 rows has to fit the 7 KB slice, so pitch <= 119 here).
// QUAD: the caller guarantees a pitch that is a multiple of four dwords and a 16-byte aligned `win`, so a lane's four dwords are all
// inside the row or all outside it and go to LDS as ONE 16-byte store.  `base` is wave-uniform and the window lies inside one plane of a
// pool below 2^31 bytes (checked at the entry), so the row address is base (scalar) + a 32-bit per-lane offset that is stepped from row
// piece to row piece: no 64-bit multiply-add per load, no multiplication at all.  The clamp of the surplus rows is taken on the offset
// (offsets grow with the row).
template <bool QUAD = false>
__device__ __forceinline__ void stage_window_rows(const uint8_t* base, uint32_t ref_stride_raw, int wrows, int pitch, uint32_t* win,
                                                  int lane)
{
    if constexpr (QUAD) {
        constexpr int NP = 6;
        typedef const __attribute__((address_space(1))) uint8_t gmem_u8;
        const int lpr = pitch >> 2;
        const int rpp = lpr < 64 ? 64 / lpr : 1;
        const int g = (int)(((uint32_t)lane * ((1u << 16) / (uint32_t)lpr + 1u)) >> 16), q4 = 4 * (lane - g * lpr);
        const bool lane_ok = g < rpp;
        gmem_u8* b = (gmem_u8*)base;
        const uint32_t step = (uint32_t)rpp * ref_stride_raw;
        const uint32_t last = (uint32_t)(wrows - 1) * ref_stride_raw + 4u * (uint32_t)q4;  // this lane's piece of the last row
        uint32_t off = (uint32_t)g * ref_stride_raw + 4u * (uint32_t)q4;
        uint32_t* o = win + g * pitch + q4;
        for (int r0 = g; r0 < wrows; r0 += NP * rpp) {
            unaligned_u32x4 w[NP];
#pragma unroll
            for (int u = 0; u < NP; u++) {
                gmem_u32x4* q = (gmem_u32x4*)(b + min(off + (uint32_t)u * step, last));
#pragma unroll
                for (int k = 0; k < 4; k++) w[u].v[k] = q->v[k];
            }
            asm volatile("" ::: "memory");  // all six loads are issued before the first store waits for one
#pragma unroll
            for (int u = 0; u < NP; u++)
                if (lane_ok && r0 < wrows - u * rpp)
                    *reinterpret_cast<u32x4_t*>(o + u * rpp * pitch) = u32x4_t{w[u].v[0], w[u].v[1], w[u].v[2], w[u].v[3]};
            off += NP * step;
            o += NP * rpp * pitch;
        }
        return;
    }
    // A lane moves FOUR consecutive dwords of a row: one 16-byte global load at the row's own byte alignment (no alignment needed on
    // this target; round 2 used five aligned dwords + four v_alignbyte) and four LDS stores.  lpr lanes per row, rpp rows per wave
    // pass, NP passes in flight: the level-1 / level-2 windows (46 / 70 rows) are then ONE round trip to memory instead of two / three
    // -- these levels spend most of their wall time waiting for this copy (tools/hme_stamps_probe.py).
    constexpr int NP = 6;
    const int lpr = (pitch + 3) >> 2;
    const int rpp = lpr < 64 ? 64 / lpr : 1;
    const int g = (int)(((uint32_t)lane * ((1u << 16) / (uint32_t)lpr + 1u)) >> 16), q4 = 4 * (lane - g * lpr);
    const bool lane_ok = g < rpp;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(base) + 4u * (uint32_t)q4;
    for (int r0 = g; r0 < wrows; r0 += NP * rpp) {
        unaligned_u32x4 w[NP];
#pragma unroll
        for (int u = 0; u < NP; u++) {
            const int r = min(r0 + u * rpp, wrows - 1);  // clamped: the loads stay unconditional and in flight together
            gmem_u32x4* q = (gmem_u32x4*)(a0 + (size_t)r * ref_stride_raw);
#pragma unroll
            for (int k = 0; k < 4; k++) w[u].v[k] = q->v[k];
        }
#pragma unroll
        for (int u = 0; u < NP; u++) {
            const int r = r0 + u * rpp;
            if (lane_ok && r < wrows) {
                uint32_t* o = win + r * pitch + q4;
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (q4 + k < pitch) o[k] = w[u].v[k];
            }
        }
    }
}

// stage_window_rows, complete and visible to the wave.  The copy is a memory round trip that the search waits for: it is issued at raised
// priority, ahead of the other waves' search loops.
template <bool QUAD>
__device__ __forceinline__ void stage_window(const uint8_t* base, uint32_t ref_stride_raw, int wrows, int pitch, uint32_t* win, int lane)
{
    HME_PRIO(3);
    stage_window_rows<QUAD>(base, ref_stride_raw, wrows, pitch, win, lane);
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    HME_PRIO(0);
}

// Window geometry of the banded LDS loops: a W-pixel block of H rows (every second plane row) over `sw` search columns, in items of `item`
// positions (8: wave_sad_loop_lds, one pad dword so that the odd pitch spreads rows over banks; 16: the level-0 loops, pitch a multiple
// of four dwords so that items stay 16-byte aligned).  `band` is the number of search rows whose window (band + 2 * H - 2 rows) fits the
// wave's slice; below 1 no band fits and the caller takes wave_sad_loop_generic.
struct HmeBands { int pitch, band; };
__device__ __forceinline__ HmeBands hme_bands(int W, int H, int sw, int item)
{
    const int pitch = (item / 4) * (int)((uint32_t)(sw + item - 1) / (uint32_t)item) + W / 4 + (item == 8 ? 1 : 0);
    return {pitch, kHmeLdsPerWave / 4 / pitch - (2 * H - 2)};
}

__device__ __forceinline__ void add_u16x4(uint32_t* sad, uint64_t acc)  // four packed u16 sums onto four 32-bit ones
{
    sad[0] += (uint32_t)acc & 0xffffu; sad[1] += ((uint32_t)acc) >> 16;
    sad[2] += (uint32_t)(acc >> 32) & 0xffffu; sad[3] += (uint32_t)(acc >> 48);
}

// SadLoopKernel by one wave for the full-SB block shapes (W = 16 / 32 / 64 px, H rows taken every second plane row), LDS-staged.  It
// takes level 1 / 2 of full SBs whose area is not the fixed shape (clipped windows, other parameters) and level 0 where the 16-position
// items do not apply (hme_level_search, hme_level0_search); the caller has checked that a band fits: hme_bands(W, H, sw, 8).band >= 1.
//   * a band of the search window is copied to this wave's LDS slice `lds` (stage_window_rows; search column 0 sits on a dword), the
//     search area is processed in bands of rows that fit;
//   * an item is 8 horizontally consecutive search positions of one search row; its lanes read W/4 + 2 window
//     dwords per block row and issue 2 * W/4 v_qsad_pk_u16_u8 (4 positions x 4 pixels each);
//   * when a level has fewer than 64 items (HME L1 / L2), RP lanes share an item and split its block rows;
//   * best position: 64-bit key (sad << 32 | raster index), lane-local strict min, then a wave min.
// `srcbuf`: the H x W source block staged by the workgroup ([H][W / 4] dwords, shared by the four region waves).
// KEY32: the caller guarantees sw * sh <= 4096 (the reference's level-1 / level-2 areas are 256 / 64 positions) and every W x H here has
// SAD < 2^20, so the best position is a 32-bit minimum of sad << 12 | position instead of a 64-bit one.
template <int W, bool KEY32 = false>
__device__ void wave_sad_loop_lds(const uint8_t* ref, uint32_t ref_stride_raw, int H, int sw, int sh, int lane, uint8_t* lds,
                                  const uint32_t* srcbuf, uint32_t* best_sad, int* bx, int* by)
{
    constexpr int WD = W / 4;                 // source dwords per block row
    constexpr int FLUSH = (W == 16) ? 16 : (W == 32 ? 8 : 4);  // rows a u16 accumulator can take: rows*W*255 < 65536
    const HmeBands g = hme_bands(W, H, sw, 8);
    const int pitch = g.pitch;                // window dwords per row
    const int band = min(g.band, sh);         // search rows per band
    uint32_t* win = reinterpret_cast<uint32_t*>(lds);

    // items and row-parts
    const int items_row = (sw + 7) >> 3;
    unsigned long long best = ~0ull;
    uint32_t best32 = 0xffffffffu;

    for (int y0 = 0; y0 < sh; y0 += band) {
        const int bh = min(band, sh - y0);
        HME_LOOP_T(t_a);
        stage_window<false>(ref + (size_t)y0 * ref_stride_raw, ref_stride_raw, bh + 2 * H - 2, pitch, win, lane);
        HME_LOOP_T(t_b);
        HME_LOOP_ADD(0, t_b, t_a);

        const int nitems = items_row * bh;
        int RP = 1, rp_shift = 0;
        while (RP < 8 && nitems * RP * 2 <= 64 && RP * 2 <= H) { RP <<= 1; rp_shift++; }
        const int ipw = 64 >> rp_shift;       // items per wave pass
        const int part = lane & (RP - 1);
        const uint32_t inv_items = (1u << 20) / (uint32_t)items_row + 1u;
        for (int it0 = 0; it0 < nitems; it0 += ipw) {
            const int item = it0 + (lane >> rp_shift);  // RP is a power of two: no per-lane integer division
            const bool valid = item < nitems;
            const int iy = valid ? (int)(((uint32_t)item * inv_items) >> 20) : 0;
            const int io = valid ? item - iy * items_row : 0;
            uint32_t sad[8];
#pragma unroll
            for (int j = 0; j < 8; j++) sad[j] = 0;
            uint64_t acc0 = 0, acc1 = 0;
            int since = 0;
            for (int r = part; r < H; r += RP) {
                const uint32_t* wr = win + (iy + 2 * r) * pitch + 2 * io;
                const uint32_t* sr = srcbuf + r * WD;
                uint32_t d[WD + 2];
#pragma unroll
                for (int c = 0; c < WD + 2; c++) d[c] = wr[c];
#pragma unroll
                for (int c = 0; c < WD; c++) {
                    const uint32_t sv = sr[c];
                    acc0 = __builtin_amdgcn_qsad_pk_u16_u8(pack64(d[c], d[c + 1]), sv, acc0);
                    acc1 = __builtin_amdgcn_qsad_pk_u16_u8(pack64(d[c + 1], d[c + 2]), sv, acc1);
                }
                if (++since == FLUSH) {
                    since = 0;
                    add_u16x4(sad, acc0);
                    add_u16x4(sad + 4, acc1);
                    acc0 = acc1 = 0;
                }
            }
            add_u16x4(sad, acc0);
            add_u16x4(sad + 4, acc1);
            // sum the row-parts of an item (its RP lanes are consecutive)
            for (int m = 1; m < RP; m <<= 1) {
#pragma unroll
                for (int j = 0; j < 8; j++) sad[j] += __shfl_xor(sad[j], m);
            }
            if (valid && part == 0) {
                const int ys = y0 + iy;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int xs = 8 * io + j;
                    if (xs < sw) {
                        if (KEY32) {
                            best32 = min(best32, (sad[j] << 12) | (uint32_t)(ys * sw + xs));
                        } else {
                            const unsigned long long key = ((unsigned long long)sad[j] << 32) | (uint32_t)(ys * sw + xs);
                            best = key < best ? key : best;  // raster order within the lane: strict '<' keeps the first
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        HME_LOOP_T(t_c);
        HME_LOOP_ADD(1, t_c, t_b);
    }
    HME_LOOP_T(t_d);
    if (KEY32)
        wave_best_u32(best32, 12, sw, best_sad, bx, by);
    else
        wave_best_u64(best, sw, best_sad, bx, by);
    HME_LOOP_T(t_e);
    HME_LOOP_ADD(2, t_e, t_d);
    HME_LOOP_ADD(3, 1ull, 0ull);
}

// Fixed-shape SadLoopKernel of HME levels 1 and 2 for full SBs whose clipped search area is the reference's whole area: level 1 a 32 x
// 16-row block over 16 x 16 positions, level 2 a 64 x 32-row block over 8 x 8 positions (every resolution class uses these).  The
// general loop above spends about 330 vector instructions per level and wave beside its 128 v_qsad per lane on run-time bands, row-part
// counts, per-row loops, u16 flushes and odd register pairs; here everything is a compile-time constant:
//   * a lane owns one whole search row (SW positions = SW / 4 accumulators of four u16 SADs) and ROWS = H / RP of the block rows; the RP
//     lanes of a search row are consecutive, their sums are combined with DPP adds;
//   * ROWS * W * 255 < 2^16: no flush, one unpack at the end;
//   * the window pitch is a multiple of four dwords, so the even window pairs (k, k + 1) arrive as aligned ds_read_b128; the odd pairs
//     are read a second time as aligned pairs (ds_read2_b32) instead of being assembled with register moves;
//   * the best position is a 32-bit (sad << 12 | raster index) minimum, the reference's strict-'<' raster rule (the KEY32 rule above).
// `srcbuf` is the block staged by the workgroup ([H][W / 4] dwords); `lds` (16-byte aligned) holds the window.
template <int W, int H, int SW, int SH>
__device__ void wave_sad_loop_fixed(const uint8_t* ref, uint32_t ref_stride_raw, int lane, uint8_t* lds, const uint32_t* srcbuf,
                                    uint32_t* best_sad, int* bx, int* by)
{
    constexpr int WD = W / 4;               // source dwords per block row
    constexpr int NQ = SW / 4;              // accumulators (position quads) per lane
    constexpr int RP = 64 / SH;             // lanes per search row
    constexpr int ROWS = H / RP;            // block rows per lane
    constexpr int ND = WD + NQ;             // window dwords a block row touches: SW + W - 1 bytes
    constexpr int PITCH = (ND + 3) & ~3;    // window dwords per row: rows stay 16-byte aligned
    constexpr int WROWS = SH + 2 * H - 2;
    static_assert(RP * SH == 64 && ROWS * RP == H && (RP & (RP - 1)) == 0 && RP >= 2 && RP <= 8, "one wave pass, RP a power of two");
    static_assert(ROWS * W * 255 < 65536 && H * W * 255 < (1 << 20) && SW * SH <= 4096 && (SW & (SW - 1)) == 0, "u16 sums, 32-bit keys");
    static_assert(WROWS * PITCH * 4 <= kHmeLdsPerWave, "the window fits the slice");
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

    uint32_t* win = reinterpret_cast<uint32_t*>(lds);
    stage_window<true>(ref, ref_stride_raw, WROWS, PITCH, win, lane);

    const int iy = lane / RP, part = lane & (RP - 1);
    const uint32_t* w0 = win + (iy + 2 * part) * PITCH;  // window row of block row `part`; block row part + RP * i is 2 * RP * i rows below
    uint64_t acc[NQ];
#pragma unroll
    for (int g = 0; g < NQ; g++) acc[g] = 0;
#pragma unroll
    for (int i = 0; i < ROWS; i++) {
        const int r = part + RP * i;
        const uint32_t* wr = w0 + 2 * RP * i * PITCH;
        // the same address as an opaque LDS pointer: the odd pairs are separate loads, not values the compiler rebuilds from the even ones
        lds_u32* wo = (lds_u32*)wr;
        asm("" : "+v"(wo));
        // the even pairs: whole 16-byte loads (kept whole by the empty asm; the compiler would otherwise split them into the 8-byte
        // pairs they feed and issue them as half-rate ds_read2_b64)
        uint32_t d[PITCH];
#pragma unroll
        for (int k = 0; k < PITCH / 4; k++) {
            if (4 * k + 2 >= ND) {  // only the first two dwords of the last quad are used (level 2)
                u32x2_t v = *reinterpret_cast<const u32x2_t*>(wr + 4 * k);
                asm("" : "+v"(v));
                d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = d[4 * k + 3] = 0;
            } else {
                u32x4_t v = *reinterpret_cast<const u32x4_t*>(wr + 4 * k);
                asm("" : "+v"(v));
                d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w;
            }
        }
        uint64_t odd[ND / 2];
#pragma unroll
        for (int k = 1; k + 1 < ND; k += 2) odd[k / 2] = pack64(wo[k], wo[k + 1]);
        uint32_t sv[WD];
#pragma unroll
        for (int k = 0; k < WD / 4; k++) {
            const uint4 v = *reinterpret_cast<const uint4*>(srcbuf + r * WD + 4 * k);
            sv[4 * k] = v.x; sv[4 * k + 1] = v.y; sv[4 * k + 2] = v.z; sv[4 * k + 3] = v.w;
        }
#pragma unroll
        for (int c = 0; c < WD; c++)
#pragma unroll
            for (int g = 0; g < NQ; g++) {
                const int k = c + g;
                acc[g] = __builtin_amdgcn_qsad_pk_u16_u8((k & 1) ? odd[k / 2] : pack64(d[k], d[k + 1]), sv[c], acc[g]);
            }
    }
    __builtin_amdgcn_wave_barrier();  // the next level's staging overwrites the window

    // per lane: min over its positions of (sad << 12 | x), after the RP lanes of the search row have added their block rows
    uint32_t key = 0xffffffffu;
#pragma unroll
    for (int g = 0; g < NQ; g++) {
        uint32_t v[4] = {(uint32_t)acc[g] & 0xffffu, (uint32_t)acc[g] >> 16, (uint32_t)(acc[g] >> 32) & 0xffffu, (uint32_t)(acc[g] >> 48)};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            v[j] += dpp_fetch<0xB1>(v[j]);                   // quad_perm [1,0,3,2]
            v[j] += dpp_fetch<0x4E>(v[j]);                   // quad_perm [2,3,0,1]
            if (RP == 8) v[j] += dpp_fetch<0x141>(v[j]);     // row_half_mirror: the other quad of the eight
        }
        key = min3u((v[0] << 12) | (uint32_t)(4 * g), (v[1] << 12) | (uint32_t)(4 * g + 1), key);
        key = min3u((v[2] << 12) | (uint32_t)(4 * g + 2), (v[3] << 12) | (uint32_t)(4 * g + 3), key);
    }
    key |= (uint32_t)(iy * SW);  // the row's raster base has no bits in common with x < SW: the lane's order is kept
    key = min(key, dpp_fetch<0xB1>(key));
    key = min(key, dpp_fetch<0x4E>(key));
    key = min(key, dpp_fetch<0x124>(key));  // row_ror:4
    key = min(key, dpp_fetch<0x128>(key));  // row_ror:8: every lane of a row of 16 holds the row's minimum
    const uint32_t best = min(min((uint32_t)__builtin_amdgcn_readlane((int)key, 0), (uint32_t)__builtin_amdgcn_readlane((int)key, 16)),
                              min((uint32_t)__builtin_amdgcn_readlane((int)key, 32), (uint32_t)__builtin_amdgcn_readlane((int)key, 48)));
    store_best(best >> 12, best & 0xfffu, (uint32_t)SW, best_sad, bx, by);
}

// One block row of a level-0 item: window dwords wr[0..7] (two ds_read_b128) against the four source dwords of the row, 16 v_qsad.
// The odd window pairs (1,2) (3,4) (5,6) are assembled in registers.  Reading them a second time from LDS as aligned pairs, as
// wave_sad_loop_fixed does, was measured and is slower here: at this loop's 16-byte lane stride every ds_read2_b32 is a four-way bank
// conflict.
__device__ __forceinline__ void l0_row_sads(const uint32_t* wr, const uint32_t* sr, uint64_t* acc)
{
    const u32x4_t da = *reinterpret_cast<const u32x4_t*>(wr);
    const u32x4_t db = *reinterpret_cast<const u32x4_t*>(wr + 4);
    const uint4 sv = *reinterpret_cast<const uint4*>(sr);
    const uint32_t d[8] = {da.x, da.y, da.z, da.w, db.x, db.y, db.z, db.w};
    const uint32_t s4[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int g = 0; g < 4; g++) acc[g] = __builtin_amdgcn_qsad_pk_u16_u8(pack64(d[c + g], d[c + g + 1]), s4[c], acc[g]);
}

// A whole level-0 item by one lane: the 8 block rows fully unrolled (128 v_qsad), so that every LDS offset is an immediate or a scalar
// multiple of the pitch.  `w0`: the item's first window row; `srcbuf`: the [8][4]-dword source block.
__device__ __forceinline__ void l0_item_sads(const uint32_t* w0, int pitch, const uint32_t* srcbuf, uint64_t* acc)
{
#pragma unroll
    for (int g = 0; g < 4; g++) acc[g] = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) l0_row_sads(w0 + 2 * r * pitch, srcbuf + r * 4, acc);
}

// Minimum of the 16 keys (sad << 16 | j), j = 0..15, of an item whose 16 positions are all valid: one v_lshl_or / v_and_or with an
// inline constant per key, one v_min3 per two keys.
__device__ __forceinline__ uint32_t l0_item_min(const uint64_t* acc)
{
    uint32_t lb = 0xffffffffu;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const uint32_t lo = (uint32_t)acc[g], hi = (uint32_t)(acc[g] >> 32);
        lb = min3u((lo << 16) | (uint32_t)(4 * g), (lo & 0xffff0000u) | (uint32_t)(4 * g + 1), lb);
        lb = min3u((hi << 16) | (uint32_t)(4 * g + 2), (hi & 0xffff0000u) | (uint32_t)(4 * g + 3), lb);
    }
    return lb;
}

// The same for the last item of a search row whose width is not a multiple of 16: only positions j < nvalid can win.
__device__ __forceinline__ uint32_t l0_item_min_masked(const uint64_t* acc, int nvalid)
{
    uint32_t lb = 0xffffffffu;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const uint32_t lo = (uint32_t)acc[g], hi = (uint32_t)(acc[g] >> 32);
        const uint32_t sad4[4] = {lo << 16, lo & 0xffff0000u, hi << 16, hi & 0xffff0000u};
#pragma unroll
        for (int j = 0; j < 4; j++) lb = min(lb, 4 * g + j < nvalid ? sad4[j] | (uint32_t)(4 * g + j) : 0xffffffffu);
    }
    return lb;
}

// Key of item `item` (search row iy of the band that starts at search row y0, nit items per row) of an area of any width: the minimum of
// its relative keys plus its raster base (y0 + iy) * sw + 16 * io.  The choice between the two minima is wave-uniform.
__device__ __forceinline__ uint32_t l0_band_item_key(const uint64_t* acc, int sw, int nit, int y0, uint32_t item, uint32_t iy)
{
    const int io = (int)(item - iy * (uint32_t)nit);
    const uint32_t lb = (sw & 15) == 0 ? l0_item_min(acc) : l0_item_min_masked(acc, sw - 16 * io);
    return lb + (uint32_t)((y0 + (int)iy) * sw + 16 * io);
}

// One remainder round of a level-0 loop: 2 / 4 / 8 lanes share an item and split its block rows, so that a handful of left-over items
// does not cost a whole 128-v_qsad pass with most lanes idle (the reference's 100 % level-0 area is 72 items: 64 + 8; the 1080p 200 %
// area 288 = 4 x 64 + 32; banded areas have a remainder per band).  The 16-bit partial sums of an item's lanes are added as packed pairs (a
// 16 x 8 SAD is < 2^16).  Takes up to 32 / 16 / 8 of the items from `it0` on and returns how many.  Every lane gets the sums `acc` of its
// item `*item` of search row `*iy` (one multiplication: at most two rounds per wave and band); `*mine`: this lane reports the item.
// The item's window address, iy * pitch + 4 * io dwords, is 4 * (item + iy) for pitch = 4 * nit + 4.
__device__ __forceinline__ int l0_remainder_round(const uint32_t* win, int pitch, const uint32_t* srcbuf, uint32_t inv_nit, int it0,
                                                  int nitems, int lane, uint64_t* acc, uint32_t* item, uint32_t* iy, bool* mine)
{
    const int rem = nitems - it0;
    const int rp_shift = rem > 16 ? 1 : rem > 8 ? 2 : 3;
    const int RP = 1 << rp_shift, take = min(rem, 64 >> rp_shift);
    const int slot = lane >> rp_shift, part = lane & (RP - 1);
    *item = (uint32_t)(it0 + min(slot, take - 1));
    *iy = (*item * inv_nit) >> 20;
    const uint32_t* w0 = win + 4u * (*item + *iy);
#pragma unroll
    for (int g = 0; g < 4; g++) acc[g] = 0;
    for (int r = part; r < 8; r += RP) l0_row_sads(w0 + 2 * r * pitch, srcbuf + r * 4, acc);
    for (int m = 1; m < RP; m <<= 1) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const uint32_t lo = (uint32_t)acc[g] + (uint32_t)__shfl_xor((int)(uint32_t)acc[g], m);
            const uint32_t hi = (uint32_t)(acc[g] >> 32) + (uint32_t)__shfl_xor((int)(uint32_t)(acc[g] >> 32), m);
            acc[g] = pack64(lo, hi);
        }
    }
    *mine = slot < take && part == 0;
    return take;
}

// Level 0 of a full SB whose clipped search width is a multiple of 16 (sw = 16 * nit) and whose whole window fits the slice in one
// band (the reference's 100 % and 200 % areas): wave_sad_loop_l0's items, passes and remainder, with what that shape makes constant.
//   * Item i of the raster of items is search row iy = i / nit, column item io = i % nit; its raster base iy * sw + 16 * io is 16 * i
//     and its window address (iy * pitch + 4 * io dwords, pitch = 4 * nit + 4) is 16 * (i + iy) bytes.  A lane computes (iy, io)
//     once and steps them from pass to pass: i + 64 is io + 64 % nit with a carry into iy.  No multiplication in the main loop.
//   * The 16 keys of an item are relative (l0_item_min); the base 16 * i is added once to the item's minimum.  It is a multiple of
//     16 and j < 16, so the sum cannot carry into the SAD field: the key stays sad << 16 | raster index, the strict-'<' raster rule.
//   * The window is staged with one 16-byte LDS store per load (stage_window_rows<true>).
// `srcbuf` is the block staged by the workgroup ([8][4] dwords); `lds` (16-byte aligned) holds the window; nit * sh * 16 <= 65536.
__device__ void wave_sad_loop_l0_oneband(const uint8_t* ref, uint32_t ref_stride_raw, int nit, int sh, int lane, uint8_t* lds,
                                         const uint32_t* srcbuf, uint32_t* best_sad, int* bx, int* by)
{
    const int pitch = 4 * nit + 4;  // hme_bands(16, 8, 16 * nit, 16).pitch
    const uint32_t* win = reinterpret_cast<const uint32_t*>(lds);
    stage_window<true>(ref, ref_stride_raw, sh + 2 * 8 - 2, pitch, reinterpret_cast<uint32_t*>(lds), lane);

    const int nitems = nit * sh;
    const uint32_t inv_nit = (1u << 20) / (uint32_t)nit + 1u;
    const uint32_t qs = (64u * inv_nit) >> 20, rs = 64u - qs * (uint32_t)nit;  // 64 = qs * nit + rs (scalar)
    uint32_t best = 0xffffffffu;
    uint32_t item = (uint32_t)lane;
    uint32_t iy = (item * inv_nit) >> 20, io = item - iy * (uint32_t)nit;
    int it0 = 0;
    // whole passes: a lane owns an item; lanes past the last item read item 0 and never win
    for (; nitems - it0 >= 57; it0 += 64) {
        const bool valid = item < (uint32_t)nitems;
        uint64_t acc[4];
        l0_item_sads(win + (valid ? 4u * (item + iy) : 0u), pitch, srcbuf, acc);
        best = min(best, valid ? l0_item_min(acc) + 16u * item : 0xffffffffu);
        item += 64;
        io += rs;
        const bool carry = io >= (uint32_t)nit;
        io -= carry ? (uint32_t)nit : 0u;
        iy += qs + (carry ? 1u : 0u);
    }
    while (it0 < nitems) {
        uint64_t acc[4];
        uint32_t ri, ry;
        bool mine;
        it0 += l0_remainder_round(win, pitch, srcbuf, inv_nit, it0, nitems, lane, acc, &ri, &ry, &mine);
        best = min(best, mine ? l0_item_min(acc) + 16u * ri : 0xffffffffu);
    }
    __builtin_amdgcn_wave_barrier();  // the next level's staging overwrites the window
    wave_best_u32(best, 16, 16 * nit, best_sad, bx, by);
}

// SadLoopKernel of HME level 0 (16 x 8-row block on the 1/16 plane; ~70 % of the search-centre work), one wave: full SBs whose width is
// not a multiple of 16 (the 140 % area, clipped windows) or whose window needs more than one band (4K, the 350 / 525 % multipliers).
// The caller (hme_level0_search) has checked hme_bands(16, 8, sw, 16).band >= 1 and sw * sh <= 65536.
// An item is 16 consecutive search positions of one search row = 16 bytes = one ds_read_b128 step along the window, so lane
// i of a row reads window dwords 4i .. 4i+7 with two conflict-free b128 loads per block row and issues 16 v_qsad_pk_u16_u8
// (4 source dwords x 4 position groups).  A 16x8 SAD is < 2^16 and the area has < 2^16 positions, so the best position is a 32-bit
// (sad << 16 | raster index) minimum, which is the reference's strict-'<' raster rule: an item's 16 keys are relative to the item
// (l0_item_min, or l0_item_min_masked where the width is not a multiple of 16: positions beyond it never win) and its raster base is
// added to their minimum, which cannot carry into the SAD field since every raster index is below 2^16.
__device__ void wave_sad_loop_l0(const uint8_t* ref, uint32_t ref_stride_raw, int sw, int sh, int lane, uint8_t* lds,
                                 const uint32_t* srcbuf, uint32_t* best_sad, int* bx, int* by)
{
    constexpr int H = 8;
    const HmeBands g = hme_bands(16, H, sw, 16);
    const int nit = (sw + 15) >> 4;                       // items per search row
    const int pitch = g.pitch, band = min(g.band, sh);
    uint32_t* win = reinterpret_cast<uint32_t*>(lds);
    uint32_t best = 0xffffffffu;
    const uint32_t inv_nit = (1u << 20) / (uint32_t)nit + 1u;
    for (int y0 = 0; y0 < sh; y0 += band) {
        const int bh = min(band, sh - y0);
        stage_window<false>(ref + (size_t)y0 * ref_stride_raw, ref_stride_raw, bh + 2 * H - 2, pitch, win, lane);
        const int nitems = nit * bh;
        int it0 = 0;
        // whole passes: a lane owns an item
        for (; nitems - it0 >= 57; it0 += 64) {
            const uint32_t item = (uint32_t)min(it0 + lane, nitems - 1);
            const uint32_t iy = (item * inv_nit) >> 20;
            uint64_t acc[4];
            l0_item_sads(win + 4u * (item + iy), pitch, srcbuf, acc);
            best = min(best, it0 + lane < nitems ? l0_band_item_key(acc, sw, nit, y0, item, iy) : 0xffffffffu);
        }
        while (it0 < nitems) {
            uint64_t acc[4];
            uint32_t item, iy;
            bool mine;
            it0 += l0_remainder_round(win, pitch, srcbuf, inv_nit, it0, nitems, lane, acc, &item, &iy, &mine);
            best = min(best, mine ? l0_band_item_key(acc, sw, nit, y0, item, iy) : 0xffffffffu);
        }
        __builtin_amdgcn_wave_barrier();
    }
    wave_best_u32(best, 16, sw, best_sad, bx, by);
}

// Level 0 of one region by one wave: a 16 x 8-row block of the 1/16 plane, `bw` pixels wide in this SB (16: a full SB, whose block the
// workgroup staged in `srcbuf`).  The one place that says which level-0 loop a shape takes.
__device__ __forceinline__ void hme_level0_search(const uint8_t* src, uint32_t src_stride, const uint8_t* ref, uint32_t ref_stride_raw, int bw,
                                                  int sw, int sh, int lane, uint8_t* lds, const uint32_t* srcbuf, uint32_t* best_sad,
                                                  int* bx, int* by)
{
    const int band16 = hme_bands(16, 8, sw, 16).band;
    if (bw == 16 && band16 >= 1 && sw * sh <= 65536) {
        if ((sw & 15) == 0 && band16 >= sh)
            wave_sad_loop_l0_oneband(ref, ref_stride_raw, sw >> 4, sh, lane, lds, srcbuf, best_sad, bx, by);
        else
            wave_sad_loop_l0(ref, ref_stride_raw, sw, sh, lane, lds, srcbuf, best_sad, bx, by);
    } else if (bw == 16 && hme_bands(16, 8, sw, 8).band >= 1) {
        wave_sad_loop_lds<16>(ref, ref_stride_raw, 8, sw, sh, lane, lds, srcbuf, best_sad, bx, by);
    } else {
        wave_sad_loop_generic(src, src_stride, ref, ref_stride_raw * 2, 8, (uint32_t)bw, ref_stride_raw, sw, sh, lane, best_sad, bx, by);
    }
}

// Level 1 or 2 of one region by one wave: a W x H-row block (32 x 16 of the 1/4 plane, 64 x 32 of the full plane), `bw` pixels wide in
// this SB (W: a full SB, whose block the workgroup staged in `srcbuf`); FSW x FSH is the reference's own area at this level, which has the
// fixed-shape loop.  The one place that says which loop a level-1 / level-2 shape takes.
template <int W, int H, int FSW, int FSH>
__device__ __forceinline__ void hme_level_search(const uint8_t* src, uint32_t src_stride, const uint8_t* ref, uint32_t ref_stride_raw, int bw,
                                                 int sw, int sh, int lane, uint8_t* lds, const uint32_t* srcbuf, uint32_t* best_sad,
                                                 int* bx, int* by)
{
    const bool fits = bw == W && hme_bands(W, H, sw, 8).band >= 1;
    if (bw == W && sw == FSW && sh == FSH)
        wave_sad_loop_fixed<W, H, FSW, FSH>(ref, ref_stride_raw, lane, lds, srcbuf, best_sad, bx, by);
    else if (fits && sw * sh <= 4096)
        wave_sad_loop_lds<W, true>(ref, ref_stride_raw, H, sw, sh, lane, lds, srcbuf, best_sad, bx, by);
    else if (fits)
        wave_sad_loop_lds<W>(ref, ref_stride_raw, H, sw, sh, lane, lds, srcbuf, best_sad, bx, by);
    else
        wave_sad_loop_generic(src, src_stride, ref, ref_stride_raw * 2, H, (uint32_t)bw, ref_stride_raw, sw, sh, lane, best_sad, bx, by);
}

__device__ __forceinline__ void clamp_center(int& x, int& y, int ox, int oy, int pw, int ph)
{
    // int16 semantics of the reference hold: every intermediate fits 16 bits for pictures <= 8K
    x = (ox + x < -63) ? (-63 - ox) : x;
    x = (ox + x > pw - 1) ? (x - ((ox + x) - (pw - 1))) : x;
    y = (oy + y < -63) ? (-63 - oy) : y;
    y = (oy + y > ph - 1) ? (y - ((oy + y) - (ph - 1))) : y;
}

// four statements per axis, each re-reading what the previous wrote (statement 2 never fires), :6690-6723
__device__ __forceinline__ void clip_window(int& xo, int& yo, int& sw, int& sh, int ox, int oy, int padw, int padh,
                                            int pw, int ph)
{
    xo = (ox + xo < -padw) ? (-padw - ox) : xo;
    sw = (ox + xo < -padw) ? (sw - (-padw - (ox + xo))) : sw;
    xo = (ox + xo > pw - 1) ? (xo - ((ox + xo) - (pw - 1))) : xo;
    sw = (ox + xo + sw > pw) ? max(1, sw - ((ox + xo + sw) - pw)) : sw;
    yo = (oy + yo < -padh) ? (-padh - oy) : yo;
    sh = (oy + yo < -padh) ? (sh - (-padh - (oy + yo))) : sh;
    yo = (oy + yo > ph - 1) ? (yo - ((oy + yo) - (ph - 1))) : yo;
    sh = (oy + yo + sh > ph) ? max(1, sh - ((oy + yo + sh) - ph)) : sh;
}

__device__ __forceinline__ int s16(int v) { return (int)(int16_t)v; }

__device__ __forceinline__ int round_hme_width(int w)
{
    return (w < 8) ? 8 : ((w & 7) ? (w + (w - ((w >> 3) << 3))) : w);  // :4528 (adds the remainder, sic)
}

struct HmeShared {
    unsigned long long cost[8];   // centre-check candidate costs
    int rx[3][4], ry[3][4];       // per level, per region ([w][h] flattened as w*2+h) centres
    unsigned long long rs[3][4];  // per level SADs (doubled)
    int cx, cy;
    unsigned long long hcost;     // CheckZeroZeroCenter cost of (cx, cy) when level 2 already computed it, else ~0
    svthip_fullpel_desc desc;     // the final descriptor, for a consumer in the same workgroup
    // source blocks of a full 64x64 SB, staged once for the four region waves: full-res rows 0,2,..,62 (64 x 32), quarter-res
    // rows 0,2,..,30 (32 x 16), sixteenth-res rows 0,2,..,14 (16 x 8)
    __attribute__((aligned(16))) uint32_t src2[32 * 16];
    __attribute__((aligned(16))) uint32_t src1[16 * 8];
    __attribute__((aligned(16))) uint32_t src0[8 * 4];
};


// Whole search-centre chain of superblock `sbi` (origin ox, oy).  Must be called by all 256 threads of the workgroup;
// `sh` and `hme_lds` (4 * kHmeLdsPerWave bytes, 16-byte aligned) are workgroup LDS.  On return (after the caller's next
// barrier) sh.desc holds the descriptor that was also written to out_desc[sbi].
__device__ __forceinline__ void hme_center_sb(const uint8_t* __restrict__ pool, const svthip_pa_picture& cur, const svthip_pa_picture& ref,
                                              const svthip_me_params& P, uint32_t list_index, int ox, int oy, uint32_t sbi,
                                              const uint32_t* __restrict__ l0_best_mv64, uint32_t l0_mv_stride,
                                              svthip_fullpel_desc* __restrict__ out_desc, int16_t* __restrict__ out_center,
                                              int16_t* __restrict__ hme_state, HmeShared& sh, uint8_t* hme_lds)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint8_t* wlds = hme_lds + wave * kHmeLdsPerWave;
    const int pw = cur.width, ph = cur.height;
    const uint32_t sb_w = (uint32_t)min(64, pw - ox), sb_h = (uint32_t)min(64, ph - oy);
    const int nw = P.number_hme_search_region_in_width, nh = P.number_hme_search_region_in_height;

    const uint8_t* cur_full = pool + cur.full_offset + (size_t)68 * cur.full_stride + 68;
    const uint8_t* ref_full = pool + ref.full_offset + (size_t)68 * ref.full_stride + 68;
    const uint8_t* src = cur_full + (size_t)oy * cur.full_stride + ox;
    HME_STAMP(0);
    HME_PRIO(3);  // until the first search loop: staging and the centre checks are a few loads and SADs on the serial path of every level

    const bool center_path = (P.temporal_layer_index > 0) || (list_index == 0);  // :6300
    const int tw = P.hme_level0_total_search_area_width, th = P.hme_level0_total_search_area_height;
    // full 64x64 SBs: stage the three source blocks once for the whole workgroup (the four region waves search with the same
    // block at every level, and the centre checks compare the same 64 x 32-row block)
    const bool full_sb = sb_w == 64 && sb_h == 64;
    // centre-check candidates 0 / B / C / D (hme_mv_center_check below, one per wave): their reference rows depend only on the SB
    // origin, so they are loaded here and stay in flight across the source-staging barrier instead of starting after it
    uint32_t cand_tv[8];
    if (full_sb && center_path) {
        int x = wave == 1 ? tw : 0, y = wave == 2 ? -th : (wave == 3 ? th : 0);
        clamp_center(x, y, ox, oy, ref.width, ref.height);
        load_ref_block64(ref_full + (size_t)(oy + y) * ref.full_stride + ox + x, ref.full_stride * 2, lane, cand_tv);
    }
    if (full_sb) {
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int i = tid + 256 * k;  // 512 dwords of the full-res block, dword aligned (SB origin multiple of 64)
            sh.src2[i] = *reinterpret_cast<const uint32_t*>(src + (size_t)(i >> 4) * (cur.full_stride * 2) + 4 * (i & 15));
        }
        if (tid < 128) {
            const uint8_t* s1 = pool + cur.quarter_offset + (size_t)(32 + (oy >> 1)) * cur.quarter_stride + 32 + (ox >> 1);
            sh.src1[tid] = ldu32_nb(s1 + (size_t)(tid >> 3) * (cur.quarter_stride * 2) + 4 * (tid & 7));
        } else if (tid < 160) {
            const int i = tid - 128;
            const uint8_t* s0 = pool + cur.sixteenth_offset + (size_t)(16 + (oy >> 2)) * cur.sixteenth_stride + 16 + (ox >> 2);
            sh.src0[i] = ldu32_nb(s0 + (size_t)(i >> 2) * (cur.sixteenth_stride * 2) + 4 * (i & 3));
        }
        __syncthreads();
    }
    const uint32_t* src2_lds = full_sb ? sh.src2 : nullptr;
    HME_STAMP(1);

    const uint32_t mv64 = (list_index == 1 && l0_best_mv64) ? l0_best_mv64[(size_t)sbi * l0_mv_stride] : 0u;
    const int dx = s16(0 - (s16((int)(mv64 & 0xffffu)) >> 2));
    const int dy = s16(0 - (s16((int)(mv64 >> 16)) >> 2));

    if (tid == 0 && hme_state && list_index == 0) hme_state[25 * (size_t)sbi + 24] = 0;
    int xc = 0, yc = 0;
    unsigned long long hme_cost = ~0ull;  // see HmeShared::hcost
    if (center_path) {
        // ---- hme_mv_center_check (:5882-6145): candidates 0 / B / C / D (+ direct for list 1); A uses the stale
        //      zero-MV index, so its cost equals the zero cost and it can never be selected before it.
        const int ncand = (list_index == 1) ? 5 : 4;
        const int cxs[5] = {0, tw, 0, 0, dx}, cys[5] = {0, 0, -th, th, dy};
        for (int c = wave; c < ncand; c += 4) {
            uint32_t sad;
            if (full_sb && c == wave) {
                sad = sad_ref_block64(cand_tv, src2_lds, lane);  // loaded before the staging barrier
            } else {
                int x = cxs[c], y = cys[c];
                clamp_center(x, y, ox, oy, ref.width, ref.height);
                sad = wave_block_sad(src, cur.full_stride * 2, ref_full + (size_t)(oy + y) * ref.full_stride + ox + x, ref.full_stride * 2,
                                     sb_h >> 1, sb_w, lane, src2_lds);
            }
            if (lane == 0) sh.cost[c] = (unsigned long long)(sad << 1) << 8;
        }
        __syncthreads();
        {
            const unsigned long long zero = sh.cost[0], b = sh.cost[1], c = sh.cost[2], d = sh.cost[3];
            const unsigned long long dir = (list_index == 1) ? sh.cost[4] : 0xFFFFFFFFFFFFFull;
            unsigned long long best = zero;
            best = b < best ? b : best;
            best = c < best ? c : best;
            best = d < best ? d : best;
            best = dir < best ? dir : best;
            if (best == zero) { xc = 0; yc = 0; }            // also covers A (same cost as zero)
            else if (best == b) { xc = tw; yc = 0; }
            else if (best == c) { xc = 0; yc = s16(0 - th); }
            else if (best == dir) { xc = dx; yc = dy; }
            else { xc = 0; yc = th; }
        }

        if (P.enable_hme_flag && sb_h == 64) {  // :6323; full height: the blocks of the three levels have 8 / 16 / 32 rows
            const int nreg = nw * nh;
            const int16_t* st = hme_state ? hme_state + 25 * (size_t)sbi : nullptr;
            const bool carried = st && list_index == 1 && st[24];
            if (wave < nreg) {
                const int rw = wave % nw, rh = wave / nw;  // visiting order h outer, w inner
                const int k = rw * 2 + rh;                 // [w][h] slot
                int x0 = xc, y0 = yc, x1 = xc, y1 = yc, x2 = xc, y2 = yc;
                if (carried) { x0 = st[k]; y0 = st[4 + k]; x1 = st[8 + k]; y1 = st[12 + k]; x2 = st[16 + k]; y2 = st[20 + k]; }
                uint32_t sad0 = 0, sad1 = 0, sad2 = 0;
                HME_STAMP(2);
                if (P.enable_hme_level0_flag) {  // HmeLevel0 :4306-4503, 1/16 picture
                    const uint32_t mx = P.hme_level0_multiplier_x, my = P.hme_level0_multiplier_y;
                    int sw = s16((int)((P.hme_level0_search_area_in_width_array[rw] * mx) / 100));
                    int shh = s16((int)((P.hme_level0_search_area_in_height_array[rh] * my) / 100));
                    int xd = s16(xc >> 2), yd = s16(yc >> 2);
                    for (int j = rw; j > 0;) { j--; xd = s16(xd + s16((int)((P.hme_level0_search_area_in_width_array[j] * mx) / 100))); }
                    for (int j = rh; j > 0;) { j--; yd = s16(yd + s16((int)((P.hme_level0_search_area_in_height_array[j] * my) / 100))); }
                    int xo = s16(-s16((int)(((tw * mx) / 100) >> 1)) + xd);
                    int yo = s16(-s16((int)(((th * my) / 100) >> 1)) + yd);
                    const int o_x = ox >> 2, o_y = oy >> 2;
                    clip_window(xo, yo, sw, shh, o_x, o_y, 15, 15, ref.width >> 2, ref.height >> 2);
                    const uint8_t* s = pool + cur.sixteenth_offset + (size_t)(16 + o_y) * cur.sixteenth_stride + 16 + o_x;
                    const uint8_t* r = pool + ref.sixteenth_offset + (size_t)(16 + o_y + yo) * ref.sixteenth_stride + 16 + o_x + xo;
                    int bx, by;
                    hme_level0_search(s, cur.sixteenth_stride * 2, r, ref.sixteenth_stride, (int)(sb_w >> 2), sw, shh, lane, wlds, sh.src0, &sad0,
                                      &bx, &by);
                    x0 = s16(s16(bx + xo) * 4);
                    y0 = s16(s16(by + yo) * 4);
                }
                HME_STAMP(3);
                if (P.enable_hme_level1_flag) {  // HmeLevel1 :4505-4625, 1/4 picture
                    int sw = round_hme_width((int)(int16_t)P.hme_level1_search_area_in_width_array[rw]);
                    int shh = (int)(int16_t)P.hme_level1_search_area_in_height_array[rh];
                    int xo = s16(-(sw >> 1) + (x0 >> 1)), yo = s16(-(shh >> 1) + (y0 >> 1));
                    const int o_x = ox >> 1, o_y = oy >> 1;
                    clip_window(xo, yo, sw, shh, o_x, o_y, 31, 31, ref.width >> 1, ref.height >> 1);
                    const uint8_t* s = pool + cur.quarter_offset + (size_t)(32 + o_y) * cur.quarter_stride + 32 + o_x;
                    const uint8_t* r = pool + ref.quarter_offset + (size_t)(32 + o_y + yo) * ref.quarter_stride + 32 + o_x + xo;
                    int bx, by;
                    hme_level_search<32, 16, 16, 16>(s, cur.quarter_stride * 2, r, ref.quarter_stride, (int)(sb_w >> 1), sw, shh, lane, wlds,
                                                     sh.src1, &sad1, &bx, &by);
                    x1 = s16(s16(bx + xo) * 2);
                    y1 = s16(s16(by + yo) * 2);
                }
                HME_STAMP(4);
                if (P.enable_hme_level2_flag) {  // HmeLevel2 :4627-4758, full resolution
                    int sw = round_hme_width((int)(int16_t)P.hme_level2_search_area_in_width_array[rw]);
                    int shh = (int)(int16_t)P.hme_level2_search_area_in_height_array[rh];
                    int xo = s16(-(sw >> 1) + x1), yo = s16(-(shh >> 1) + y1);
                    clip_window(xo, yo, sw, shh, ox, oy, 63, 63, ref.width, ref.height);
                    const uint8_t* r = ref_full + (size_t)(oy + yo) * ref.full_stride + ox + xo;
                    int bx, by;
                    hme_level_search<64, 32, 8, 8>(src, cur.full_stride * 2, r, ref.full_stride, (int)sb_w, sw, shh, lane, wlds, sh.src2, &sad2,
                                                   &bx, &by);
                    x2 = s16(bx + xo);
                    y2 = s16(by + yo);
                }
                HME_STAMP(5);
                if (lane == 0) {
                    sh.rx[0][k] = x0; sh.ry[0][k] = y0; sh.rs[0][k] = (unsigned long long)sad0 * 2;
                    sh.rx[1][k] = x1; sh.ry[1][k] = y1; sh.rs[1][k] = (unsigned long long)sad1 * 2;
                    sh.rx[2][k] = x2; sh.ry[2][k] = y2; sh.rs[2][k] = (unsigned long long)sad2 * 2;
                }
            }
            __syncthreads();
            if (tid == 0) {
                // region pick (:6510-6631): start at [0][0], then w-inner order from w = 1, strict '<'
                int lvl = -1;
                if (P.enable_hme_level0_flag && !P.enable_hme_level1_flag && !P.enable_hme_level2_flag) lvl = 0;
                if (P.enable_hme_level1_flag && !P.enable_hme_level2_flag) lvl = 1;
                if (P.enable_hme_level2_flag) lvl = 2;
                int xh = 0, yh = 0;
                unsigned long long bs = ~0ull;
                if (lvl >= 0) {
                    xh = sh.rx[lvl][0]; yh = sh.ry[lvl][0];
                    bs = sh.rs[lvl][0];
                    int w = 1, h = 0;
                    while (h < nh) {
                        while (w < nw) {
                            const int k = w * 2 + h;
                            if (sh.rs[lvl][k] < bs) { xh = sh.rx[lvl][k]; yh = sh.ry[lvl][k]; bs = sh.rs[lvl][k]; }
                            w++;
                        }
                        w = 0;
                        h++;
                    }
                }
                // The level-2 SAD of the chosen centre is the SAD CheckZeroZeroCenter compares: the same 64 x 32-row block at the same
                // position, and clip_window(.., 63, 63, ref size) keeps every level-2 position inside clamp_center's range, so its clamp
                // leaves the centre where it is.  rs[2] = 2 * SAD; the check's cost is (SAD << 1) << 8.
                unsigned long long hcost = lvl == 2 ? bs << 8 : ~0ull;
                if (P.enable_hme_level2_flag) {
                    const int total = nh * nw;
                    if (P.ref_poc_equal && list_index == 1 && total > 1) {
                        // bubble sort by SAD with the reference's [q / nw][q % nw] indexing, then take [0][1] (:6606-6631).  That indexing
                        // can reach slots of regions that do not exist; `from` follows where each entry came from, so that only a
                        // searched region's SAD is handed on as the centre's cost
                        uint32_t from = 0xE4u;  // 2-bit origin slot of each entry: [3, 2, 1, 0]
                        for (int q = 0; q < total - 1; q++)
                            for (int n = q + 1; n < total; n++) {
                                const int a = (q / nw) * 2 + (q % nw), b = (n / nw) * 2 + (n % nw);
                                if (sh.rs[2][a] > sh.rs[2][b]) {
                                    const int tx = sh.rx[2][a], ty = sh.ry[2][a];
                                    const uint32_t fa = (from >> (2 * a)) & 3u, fb = (from >> (2 * b)) & 3u;
                                    const unsigned long long ts = sh.rs[2][a];
                                    sh.rx[2][a] = sh.rx[2][b]; sh.ry[2][a] = sh.ry[2][b]; sh.rs[2][a] = sh.rs[2][b];
                                    sh.rx[2][b] = tx; sh.ry[2][b] = ty; sh.rs[2][b] = ts;
                                    from ^= ((fa ^ fb) << (2 * a)) | ((fa ^ fb) << (2 * b));
                                }
                            }
                        xh = sh.rx[2][1];
                        yh = sh.ry[2][1];
                        const uint32_t f1 = (from >> 2) & 3u;
                        const bool live = (int)(f1 >> 1) < nw && (int)(f1 & 1u) < nh;
                        hcost = live ? sh.rs[2][1] << 8 : ~0ull;
                    }
                }
                sh.cx = xh;
                sh.cy = yh;
                sh.hcost = hcost;
                if (hme_state) {
                    int16_t* so = hme_state + 25 * (size_t)sbi;
                    for (int k = 0; k < 4; k++) {
                        // regions that do not exist keep the initial centre, like the reference's arrays
                        const bool live = ((k >> 1) < nw) && ((k & 1) < nh);
                        for (int l = 0; l < 3; l++) {
                            so[8 * l + k] = (int16_t)(live ? sh.rx[l][k] : (carried ? so[8 * l + k] : 0));
                            so[8 * l + 4 + k] = (int16_t)(live ? sh.ry[l][k] : (carried ? so[8 * l + 4 + k] : 0));
                        }
                    }
                    so[24] = 1;
                }
            }
            __syncthreads();
            xc = sh.cx;
            yc = sh.cy;
            hme_cost = sh.hcost;
        }
    }

    // ---- CheckZeroZeroCenter (:5466-5552) ----
    HME_PRIO(3);
    if ((xc != 0 || yc != 0) && P.is_used_as_reference_flag) {
        clamp_center(xc, yc, ox, oy, ref.width, ref.height);
        unsigned long long z, hcost;
        if (hme_cost != ~0ull && ox < ref.width && oy < ref.height) {
            // both SADs are known: the zero vector is centre-check candidate 0 (the same block; clamp_center leaves (0, 0) in place
            // inside the reference picture), the centre's is its level-2 SAD
            z = sh.cost[0];
            hcost = hme_cost;
        } else {
            __syncthreads();
            if (wave < 2) {
                const int x = wave ? xc : 0, y = wave ? yc : 0;
                const uint32_t sad = wave_block_sad(src, cur.full_stride * 2, ref_full + (size_t)(oy + y) * ref.full_stride + ox + x,
                                                    ref.full_stride * 2, sb_h >> 1, sb_w, lane, src2_lds);
                if (lane == 0) sh.cost[6 + wave] = (unsigned long long)(sad << 1) << 8;
            }
            __syncthreads();
            z = sh.cost[6];
            hcost = sh.cost[7];
        }
        const unsigned long long m = z < hcost ? z : hcost;
        if (m == z) { xc = 0; yc = 0; }
    }

    HME_STAMP(6);
    if (tid == 0) {
        int sw = min((int)P.search_area_width, 127), shh = min((int)P.search_area_height, 127);
        int xo = s16(xc - (sw >> 1)), yo = s16(yc - (shh >> 1));
        clip_window(xo, yo, sw, shh, ox, oy, 63, 63, pw, ph);
        svthip_fullpel_desc d;
        d.src_offset = (int32_t)(cur.full_offset + (int64_t)(68 + oy) * cur.full_stride + 68 + ox);
        d.ref_offset = (int32_t)(ref.full_offset + (int64_t)(68 + oy + yo) * ref.full_stride + 68 + ox + xo);
        d.x_search_area_origin = xo;
        d.y_search_area_origin = yo;
        d.search_area_width = sw;
        d.search_area_height = shh;
        out_desc[sbi] = d;
        sh.desc = d;
        if (out_center) {
            out_center[2 * sbi] = (int16_t)xc;
            out_center[2 * sbi + 1] = (int16_t)yc;
        }
    }
}
