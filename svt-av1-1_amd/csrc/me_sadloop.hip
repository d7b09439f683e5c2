// svt-av1-1_amd/csrc/me_sadloop.hip
//
// SadLoopKernel for a batch of blocks, gfx950: exhaustive SAD search of one W x H block over a search_area_width x
// search_area_height grid, first minimum in raster order (strict '<').  Replaces NxMSadLoopKernel_funcPtrArray[asm_type]
// (Source/Lib/Codec/EbComputeSAD.h:183-189) = SadLoopKernel (C_DEFAULT/EbComputeSAD_C.c:73-119), SadLoopKernel_SSE4_1_INTRIN /
// _AVX2_INTRIN, the kernel behind HmeLevel0/1/2 (Codec/EbMotionEstimation.c:4306-4758) and BASELINE configs[0]
// (16x16 blocks, +-16, 856x480).  The hierarchical-ME kernel (me_hme_impl.h) has its own specialised copies for the three HME
// block shapes; this is the generic entry with the reference's full argument set (row-skipping strides included).
//
// One wave per block, four blocks per 256-thread workgroup.  The block and its reference window live in a per-wave LDS slice; a lane
// owns search positions p = lane, lane + 64, ... (raster order); per 4 block pixels: one broadcast ds_read of the source dword, an
// unaligned window dword (two aligned reads + v_alignbyte) and one v_sad_u8.  Best = min over (sad << 12 | p): the first minimum in
// raster order, exactly the reference's strict-'<' update; DPP / readlane reduction over the wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "me_launch.h"
#include "me_sad_common.h"

namespace svthip {

namespace {

typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) uint32_t lds_u32;

__device__ __forceinline__ uint32_t lds_u32_at(const lds_u8* p)
{
    const uint32_t a = (uint32_t)reinterpret_cast<uintptr_t>(p);
    const lds_u32* q = reinterpret_cast<const lds_u32*>((uintptr_t)(a & ~3u));
    return __builtin_amdgcn_alignbyte(q[1], q[0], a & 3u);
}

}  // namespace

__global__ void __launch_bounds__(256) sad_loop_kernel(const uint8_t* __restrict__ src, uint32_t src_stride, const uint8_t* __restrict__ ref,
                                                       uint32_t ref_stride, uint32_t ref_stride_raw, const svthip_sad_loop_desc* __restrict__ desc,
                                                       uint32_t n_blocks, int w, int h, int sw, int sh, int slice_bytes,
                                                       uint32_t* __restrict__ best_sad, int16_t* __restrict__ best_xy)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t b = blockIdx.x * 4 + wave;
    if (b >= n_blocks) return;  // whole wave; no workgroup barrier below
    lds_u8* blk = (lds_u8*)smem + wave * slice_bytes;  // [h][w] source block, then the window
    lds_u8* win = blk + h * w;
    const int k = (int)(ref_stride / ref_stride_raw);                // rows of the plane between two block rows (1, or 2 when rows are skipped)
    const int wrows = (sh - 1) + (h - 1) * k + 1, wcols = w + sw - 1;
    const int pitch = (wcols + 3 + 4) & ~3;                          // +4: the unaligned dword read of the last columns
    const svthip_sad_loop_desc d = desc[b];
    const int w4 = w >> 2;
    for (int i = lane; i < h * w4; i += 64) {
        const int y = i / w4, x = 4 * (i - y * w4);
        const uint8_t* p = src + d.src_offset + (size_t)y * src_stride + x;
        reinterpret_cast<lds_u32*>(blk)[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
    {
        const uint8_t* base = ref + d.ref_offset;
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(base);
        const uint32_t shf = (uint32_t)(a0 & 3u);
        const int ndw = pitch >> 2;
        for (int i = lane; i < wrows * ndw; i += 64) {
            const int r = i / ndw, c = i - r * ndw;
            // aligned dword pair of row r (the plane's raw stride may be odd: re-derive the alignment per row)
            const uintptr_t a = a0 + (size_t)r * ref_stride_raw + 4 * c;
            const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
            reinterpret_cast<lds_u32*>(win)[i] = 4 * c < wcols + 3 ? __builtin_amdgcn_alignbyte(q[1], q[0], (uint32_t)(a & 3u)) : 0u;
            (void)shf;
        }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    uint32_t best = 0xffffffffu;
    const int n_pos = sw * sh;
    for (int p = lane; p < n_pos; p += 64) {
        const int ys = p / sw, xs = p - ys * sw;
        uint32_t sad = 0;
        const lds_u8* wp = win + ys * pitch + xs;
        for (int y = 0; y < h; y++) {
            const lds_u32* srow = reinterpret_cast<const lds_u32*>(blk + y * w);
            const lds_u8* rrow = wp + y * k * pitch;
#pragma unroll 4
            for (int x4 = 0; x4 < w4; x4++) sad = __builtin_amdgcn_sad_u8(srow[x4], lds_u32_at(rrow + 4 * x4), sad);
        }
        const uint32_t key = (sad << 12) | (uint32_t)p;
        best = key < best ? key : best;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)best, m);
        best = o < best ? o : best;
    }
    if (lane == 0) {
        const int p = (int)(best & 0xfffu);
        best_sad[b] = best >> 12;
        best_xy[2 * b] = (int16_t)(p % sw);
        best_xy[2 * b + 1] = (int16_t)(p / sw);
    }
}

// Packed-SAD path for block widths 4 / 8 / 16 / 32 / 64 (W4 = width / 4 dwords), round 3: a 256-thread WORKGROUP owns `gb` blocks.
//   * a lane owns 4 * NQ consecutive positions of one search row: per source dword NQ v_qsad_pk_u16_u8 (positions 4 n .. 4 n + 3 on the
//     window dword pair (j + n, j + n + 1)) -- 16 abs-diff per instruction.  NQ (2, 3 or 4) is the one that pads the search width least:
//     the 33 columns of configs[0] take 36 positions with NQ = 3 (40 with the eight-position form of round 2);
//   * the items (block, search row, position group) of all gb blocks are dealt out over the 256 lanes as one flat list, so the last
//     round of 64 lanes is shared by the blocks instead of being paid per block: 5 blocks x 99 items = 495 of 512 lane slots
//     (one block per wave: 165 of 192); gb is chosen on the host for the fewest empty slots within the LDS budget;
//   * a lane's best key goes to its block's LDS word with one ds_min_u32 per item; key = sad << 12 | raster position, so the minimum is
//     the first minimum in raster order, the reference's strict-'<' update (C_DEFAULT/EbComputeSAD_C.c:73-119).
// The packed 16-bit sums are widened every 256 / width rows (a row adds at most width / 4 * 1020 per position).
// LDS image of a block's window: rows of `pitch` bytes; a group starts 4 * NQ bytes after its neighbour and is read with ds_read_b64 (NQ = 2) /
// ds_read_b128 (NQ = 4) at 256 B/clk, or ds_read2_b32 (NQ = 3: a 12-position group can start on an odd dword).  A chunk-major "cell" image
// that gave the 12-position groups ds_read_b128 too halved the LDS cycles (counters) but cost more staging instructions than it saved: dropped.
struct SadLoopPlan {
    int nq, gb, pitch, slice_bytes;
    size_t lds_bytes;
};

inline SadLoopPlan sad_loop_plan(int w, int h, int sw, int sh, int k)
{
    SadLoopPlan p{};
    int best_cols = 1 << 30;
    for (int nq = 4; nq >= 2; nq--) {  // ties go to the larger group: fewer LDS reads per v_qsad
        const int cols = 4 * nq * ((sw + 4 * nq - 1) / (4 * nq));
        if (cols < best_cols) best_cols = cols, p.nq = nq;
    }
    // a row holds every group's width / 4 + nq dwords (zero beyond the window); rows are 16-byte units (staged with ds_write_b128), an odd
    // number of them so that neighbouring search rows start on different banks
    int pitch = (best_cols + w + 15) & ~15;
    if (!((pitch >> 4) & 1)) pitch += 16;
    p.pitch = pitch;
    const int wrows = (sh - 1) + (h - 1) * k + 1, ng = (sw + 4 * p.nq - 1) / (4 * p.nq);
    const int blk_bytes = (h * w + 15) & ~15;
    p.slice_bytes = blk_bytes + wrows * pitch;
    const int ipb = ng * sh;
    // blocks per workgroup: the fewest that fill the lane slots of the last round (within 2 %), inside 40 KB of LDS (four workgroups per CU)
    p.gb = 1;
    double best_util = (double)ipb / (256.0 * ((ipb + 255) / 256));
    for (int g = 2; g <= 16; g++) {
        if (192 + (size_t)g * p.slice_bytes > 40 * 1024) break;
        const int rounds = (g * ipb + 255) / 256;
        const double util = (double)(g * ipb) / (256.0 * rounds);
        if (util > best_util + 0.02) best_util = util, p.gb = g;
    }
    p.lds_bytes = 192 + (size_t)p.gb * p.slice_bytes;
    return p;
}

template <int W4, int NQ>
__global__ void __launch_bounds__(256) sad_loop_qsad_kernel(const uint8_t* __restrict__ src, uint32_t src_stride, const uint8_t* __restrict__ ref,
                                                            uint32_t ref_stride, uint32_t ref_stride_raw,
                                                            const svthip_sad_loop_desc* __restrict__ desc, uint32_t n_blocks, int h, int sw, int sh,
                                                            int gb, int slice_bytes, int pitch, uint32_t* __restrict__ best_sad,
                                                            int16_t* __restrict__ best_xy)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int w = 4 * W4, PPL = 4 * NQ, NW = W4 + NQ;  // NW window dwords per lane and block row
    constexpr int CH = (NW + 3) / 4;                       // 16-byte chunks a lane reads per window row (NQ = 4)
    constexpr int FL = 256 / w;                            // rows between two widenings
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) u32x2 lds_u32x2;
    typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
    const int tid = threadIdx.x;
    const uint32_t b0 = blockIdx.x * (uint32_t)gb;
    const int nb = (int)min((uint32_t)gb, n_blocks - b0);
    lds_u32* lds_best = reinterpret_cast<lds_u32*>((lds_u8*)smem);  // [16]
    lds_u8* slices = (lds_u8*)smem + 192;
    const int k = (int)(ref_stride / ref_stride_raw);
    const int ng = (sw + PPL - 1) / PPL;
    const int wrows = (sh - 1) + (h - 1) * k + 1, wcols = w + sw - 1;
    const int blk_bytes = (h * w + 15) & ~15;
    // header: best keys [16], then the descriptors of the workgroup's blocks [16]
    lds_u32* lds_desc = lds_best + 16;
    if (tid < 16) lds_best[tid] = 0xffffffffu;
    if (tid < nb) {
        const svthip_sad_loop_desc d = desc[b0 + tid];
        lds_desc[2 * tid] = d.src_offset;
        lds_desc[2 * tid + 1] = d.ref_offset;
    }
    __syncthreads();
    // ---- stage the nb source blocks and windows (global loads at byte alignment; nothing is read beyond the dword that holds the window's
    //      last column).  A thread stages whole ROWS: the address arithmetic (two reciprocal divisions, a 64-bit row address) is paid once per
    //      row instead of once per 16-byte unit -- per unit it made staging 40 % of the kernel's vector instructions. ----
    {
        const int ndw_valid = (wcols + 3) >> 2, qpr = pitch >> 4;
        const uint32_t inv_wrows = (uint32_t)((0x100000000ull + (uint32_t)wrows - 1u) / (uint32_t)wrows);
        for (int u = tid; u < nb * wrows; u += 256) {
            const int bi = wrows == 1 ? u : (int)__umulhi((uint32_t)u, inv_wrows), r = u - bi * wrows;
            const uint8_t* p = ref + lds_desc[2 * bi + 1] + (size_t)r * ref_stride_raw;
            lds_u32x4* wq = reinterpret_cast<lds_u32x4*>(slices + bi * slice_bytes + blk_bytes + r * pitch);
            for (int c = 0; c < qpr; c++) {
                const int left = ndw_valid - 4 * c;
                uint32_t t[4] = {0u, 0u, 0u, 0u};
                if (left >= 4) {
                    const unaligned_u32x4 v = *reinterpret_cast<const unaligned_u32x4*>(p + 16 * c);
                    t[0] = v.v[0]; t[1] = v.v[1]; t[2] = v.v[2]; t[3] = v.v[3];
                } else if (left > 0) {
#pragma unroll
                    for (int q = 0; q < 3; q++)
                        if (q < left) t[q] = reinterpret_cast<const unaligned_u32*>(p + 16 * c + 4 * q)->v;
                }
                wq[c] = u32x4{t[0], t[1], t[2], t[3]};
            }
        }
        const uint32_t inv_h = (uint32_t)((0x100000000ull + (uint32_t)h - 1u) / (uint32_t)h);
        for (int u = tid; u < nb * h; u += 256) {
            const int bi = h == 1 ? u : (int)__umulhi((uint32_t)u, inv_h), y = u - bi * h;
            const uint8_t* p = src + lds_desc[2 * bi] + (size_t)y * src_stride;
            lds_u32* sq = reinterpret_cast<lds_u32*>(slices + bi * slice_bytes + y * w);
#pragma unroll
            for (int x = 0; x < W4; x++) sq[x] = reinterpret_cast<const unaligned_u32*>(p + 4 * x)->v;
        }
    }
    __syncthreads();

    const int ipb = ng * sh, total = nb * ipb;
    const uint32_t inv_ipb = (uint32_t)((0x100000000ull + (uint32_t)ipb - 1u) / (uint32_t)ipb);
    const uint32_t inv_ng = (uint32_t)((0x100000000ull + (uint32_t)ng - 1u) / (uint32_t)ng);
    const int rstep = k * pitch;  // bytes between the window rows of two block rows
    for (int t = tid; t < total; t += 256) {
        // t / ipb and it / ng by reciprocal (exact below 2^16; a divisor of 1 has no 32-bit reciprocal)
        const int bi = ipb == 1 ? t : (int)__umulhi((uint32_t)t, inv_ipb), it = t - bi * ipb;
        const int ys = ng == 1 ? it : (int)__umulhi((uint32_t)it, inv_ng), xg = it - ys * ng, x0 = PPL * xg;
        const lds_u8* blk = slices + bi * slice_bytes;
        const lds_u8* sp = blk;
        const lds_u8* wp = blk + blk_bytes + ys * pitch + x0;
        uint32_t sum[PPL];
#pragma unroll
        for (int i = 0; i < PPL; i++) sum[i] = 0;
        for (int y0 = 0; y0 < h; y0 += FL) {
            uint64_t acc[NQ];
#pragma unroll
            for (int n = 0; n < NQ; n++) acc[n] = 0;
            const int y1 = min(h, y0 + FL);
#pragma unroll 2
            for (int y = y0; y < y1; y++) {
                const lds_u8* rrow = wp + y * rstep;
                uint32_t Wd[4 * CH + 4], S[W4];
                if constexpr (NQ == 4) {  // x0 and the pitch are multiples of 16
#pragma unroll
                    for (int c = 0; c < CH; c++) {
                        const u32x4 v = reinterpret_cast<const lds_u32x4*>(rrow)[c];
                        Wd[4 * c] = v.x; Wd[4 * c + 1] = v.y; Wd[4 * c + 2] = v.z; Wd[4 * c + 3] = v.w;
                    }
                } else if constexpr (NQ == 2) {  // x0 and the pitch are multiples of 8
#pragma unroll
                    for (int c = 0; c < (NW + 1) / 2; c++) {
                        const u32x2 v = reinterpret_cast<const lds_u32x2*>(rrow)[c];
                        Wd[2 * c] = v.x; Wd[2 * c + 1] = v.y;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < NW; j++) Wd[j] = reinterpret_cast<const lds_u32*>(rrow)[j];
                }
                const lds_u8* srow = sp + y * w;  // 4 * W4 bytes per block row, the block 16-byte aligned
                if constexpr (W4 >= 4) {
#pragma unroll
                    for (int c = 0; c < W4 / 4; c++) {
                        const u32x4 v = reinterpret_cast<const lds_u32x4*>(srow)[c];
                        S[4 * c] = v.x; S[4 * c + 1] = v.y; S[4 * c + 2] = v.z; S[4 * c + 3] = v.w;
                    }
                } else if constexpr (W4 == 2) {
                    const u32x2 v = *reinterpret_cast<const lds_u32x2*>(srow);
                    S[0] = v.x; S[1] = v.y;
                } else {
                    S[0] = *reinterpret_cast<const lds_u32*>(srow);
                }
#pragma unroll
                for (int j = 0; j < W4; j++)
#pragma unroll
                    for (int n = 0; n < NQ; n++)
                        acc[n] = __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)Wd[j + n + 1] << 32) | Wd[j + n], S[j], acc[n]);
            }
#pragma unroll
            for (int n = 0; n < NQ; n++) {
                sum[4 * n + 0] += (uint32_t)acc[n] & 0xffffu;
                sum[4 * n + 1] += ((uint32_t)acc[n]) >> 16;
                sum[4 * n + 2] += (uint32_t)(acc[n] >> 32) & 0xffffu;
                sum[4 * n + 3] += (uint32_t)(acc[n] >> 48);
            }
        }
        const uint32_t p0 = (uint32_t)(ys * sw + x0);
        uint32_t best = 0xffffffffu;
#pragma unroll
        for (int i = 0; i < PPL; i++) {
            const uint32_t key = (x0 + i < sw) ? ((sum[i] << 12) | (p0 + i)) : 0xffffffffu;
            best = key < best ? key : best;
        }
        __hip_atomic_fetch_min(reinterpret_cast<uint32_t*>(smem) + bi, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (tid < nb) {
        const uint32_t best = lds_best[tid];
        const int p = (int)(best & 0xfffu);
        best_sad[b0 + tid] = best >> 12;
        best_xy[2 * (b0 + tid)] = (int16_t)(p % sw);
        best_xy[2 * (b0 + tid) + 1] = (int16_t)(p / sw);
    }
}

namespace {

// the packed-SAD kernel takes this shape, with plan *p: a width it has a form for, not overridden, and a plan within the default dynamic
// LDS limit (its window rows are slightly wider than the generic kernel's)
bool sad_loop_takes_qsad(int w, int h, int sw, int sh, int k, bool force_generic, SadLoopPlan* p)
{
    if (!(w == 4 || w == 8 || w == 16 || w == 32 || w == 64) || force_generic) return false;
    *p = sad_loop_plan(w, h, sw, sh, k);
    return p->lds_bytes <= 64 * 1024;
}

hipError_t launch_sad_loop_qsad(const uint8_t* src, uint32_t src_stride, const uint8_t* ref, uint32_t ref_stride, uint32_t ref_stride_raw,
                                const svthip_sad_loop_desc* desc, uint32_t n_blocks, int w, int h, int sw, int sh, const SadLoopPlan& p,
                                uint32_t* best_sad, int16_t* best_xy, hipStream_t s)
{
    const dim3 grid((n_blocks + p.gb - 1) / p.gb), block(256);
#define SVTHIP_SADLOOP_CASE(W4, NQ)                                                                                                         \
    case 16 * W4 + NQ:                                                                                                                      \
        hipLaunchKernelGGL((sad_loop_qsad_kernel<W4, NQ>), grid, block, p.lds_bytes, s, src, src_stride, ref, ref_stride, ref_stride_raw, desc, \
                           n_blocks, h, sw, sh, p.gb, p.slice_bytes, p.pitch, best_sad, best_xy);                                          \
        break;
#define SVTHIP_SADLOOP_W(W4) SVTHIP_SADLOOP_CASE(W4, 2) SVTHIP_SADLOOP_CASE(W4, 3) SVTHIP_SADLOOP_CASE(W4, 4)
    switch (4 * w + p.nq) {
        SVTHIP_SADLOOP_W(1)
        SVTHIP_SADLOOP_W(2)
        SVTHIP_SADLOOP_W(4)
        SVTHIP_SADLOOP_W(8)
        SVTHIP_SADLOOP_W(16)
    default: return hipErrorInvalidValue;
    }
#undef SVTHIP_SADLOOP_W
#undef SVTHIP_SADLOOP_CASE
    return hipGetLastError();
}

// LDS of one block of the generic kernel (a workgroup holds four)
size_t sad_loop_slice_bytes(int w, int h, int sw, int sh, int k)
{
    const int wrows = (sh - 1) + (h - 1) * k + 1, pitch = (w + sw - 1 + 3 + 4) & ~3;
    return ((size_t)h * w + (size_t)wrows * pitch + 15) & ~(size_t)15;
}

}  // namespace

bool sad_loop_fits(int w, int h, int sw, int sh, int k, bool force_generic, size_t* generic_slice_bytes)
{
    SadLoopPlan p;
    if (sad_loop_takes_qsad(w, h, sw, sh, k, force_generic, &p)) return true;
    *generic_slice_bytes = sad_loop_slice_bytes(w, h, sw, sh, k);
    return *generic_slice_bytes * 4 <= 64 * 1024;
}

hipError_t launch_sad_loop(const uint8_t* src, uint32_t src_stride, const uint8_t* ref, uint32_t ref_stride, uint32_t ref_stride_raw,
                           const svthip_sad_loop_desc* desc, uint32_t n_blocks, int w, int h, int sw, int sh, bool force_generic, uint32_t* best_sad,
                           int16_t* best_xy, hipStream_t s)
{
    const int k = (int)(ref_stride / ref_stride_raw);
    SadLoopPlan p;
    if (sad_loop_takes_qsad(w, h, sw, sh, k, force_generic, &p))
        return launch_sad_loop_qsad(src, src_stride, ref, ref_stride, ref_stride_raw, desc, n_blocks, w, h, sw, sh, p, best_sad, best_xy, s);
    const size_t slice = sad_loop_slice_bytes(w, h, sw, sh, k);
    hipLaunchKernelGGL(sad_loop_kernel, dim3((n_blocks + 3) / 4), dim3(256), slice * 4, s, src, src_stride, ref, ref_stride, ref_stride_raw, desc, n_blocks,
                       w, h, sw, sh, (int)slice, best_sad, best_xy);
    return hipGetLastError();
}

}  // namespace svthip
