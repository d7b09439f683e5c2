// svt-av1-1_amd/csrc/ip_warp.hip
//
// Warped-motion (WARPED_CAUSAL) inter prediction of whole PUs: Y, Cb and Cr of a batch of prediction units of one luma size, each what
// one call of warped_motion_prediction writes (Source/Lib/Codec/EbInterPrediction.c:2528-2861): av1_warp_affine_c /
// av1_highbd_warp_affine_c (Codec/EbWarpedMotion.c:672-798 / :389-511) on luma and, for blocks of at least 16x16, on both chroma planes;
// for smaller blocks a translational chroma prediction with interp_filters = 0.
//
//   warp       warp_kernel: one 8x8 output block of one plane per wave, sixteen blocks per workgroup (four per wave).  A PU of bw x bh is
//              (bw / 8)(bh / 8) luma blocks plus, when its chroma is warped, 2 (bw / 16)(bh / 16) chroma blocks, so the grid is known on
//              the host and a block finds its PU by a division.  The block centre, ix4 / sx4 / iy4 / sy4 are wave-uniform.  The 15 x 8
//              horizontal results (two passes of the wave) go to LDS as 16-bit values (< 2^13 at 8 bits, < 2^15 at 10), the vertical
//              pass is one lane per output sample.  The filter row is chosen per sample from the 193-row table, staged in LDS as packed
//              bytes (1 544 bytes); 8-bit horizontal sums are ip_common.h's dot8 on (pixel - 128) bytes, the bias folded into the offset
//              (rows sum to 128).  Source rows: when the block's 15 x 15 window (and the dwords around it) lies inside the picture,
//              aligned dwords + v_alignbyte; otherwise per-sample coordinates clamped to the picture as the reference clamps them.
//              The choice is wave-uniform.
//   chroma < 8x8   warp_chroma_expand_kernel writes one job per PU in the format of the counted convolution kernels (ip_convolve.hip,
//              COUNTED), which then run unchanged on Cb and Cr: clamp_mv_to_umv_border_sb(xd, mv, bwidth_uv, bheight_uv, 1, 1), source at
//              ((pu_origin >> 3) << 3) / 2, filters 0 / 0 -- the clamp, geometry and job word of ip_common.h, as in ip_inter_pred.hip.
//
// A PU whose model fails the reference's validity tests (is_affine_valid, is_affine_shear_allowed, Codec/EbWarpedMotion.c:329-341: the
// filter-row index would leave [0, 192]), whose wmtype is not ROTZOOM / AFFINE, or whose translational chroma block would start outside the
// border its edges describe, is refused: nothing is written for it and the context's counter is incremented once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svtav1_hip.h"
#include "ip_common.h"
#include "ip_launch.h"

static_assert(sizeof(svthip_warp_pu_desc) == 64, "svthip_warp_pu_desc is 64 bytes (include/svtav1_hip.h)");

namespace svthip {

namespace {

// [row 0..192][taps 0-3, taps 4-7] as packed signed bytes
__device__ const uint32_t kWarpFilter[193][2] =
#include "av1_warp_filter.inc"
    ;

constexpr int kBlocksPerWave = 4, kBlocksPerGroup = 4 * kBlocksPerWave;

struct WarpArgs {
    const uint8_t *ry, *rcb, *rcr;  // reference planes at picture sample (0, 0)
    uint8_t *dy, *dcb, *dcr;
    uint32_t rys, rcs, dys, dcs;    // strides in samples
    int pic_w, pic_h;
    int bw, bh;
    int warp_chroma;                // bw >= 16 && bh >= 16
    int bd;
    int64_t kc;                     // rebasing of the chroma source planes for the translational jobs, in samples
};

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

// is_affine_valid / is_affine_shear_allowed, and the model types warp_plane accepts
__device__ __forceinline__ bool model_valid(const svthip_warp_pu_desc& d)
{
    if (d.wmtype != 2 && d.wmtype != 3) return false;
    if (d.wmmat[2] <= 0) return false;
    if (4 * iabs(d.alpha) + 7 * iabs(d.beta) >= (1 << 16)) return false;
    if (4 * iabs(d.gamma) + 4 * iabs(d.delta) >= (1 << 16)) return false;
    return true;
}

// The translational chroma job of a PU smaller than 16x16: clamp_mv_to_umv_border_sb with (bwidth_uv, bheight_uv, 1, 1), integer /
// fraction split, offsets.  false: the block would start outside the rebased range (edges that do not describe the PU's position).
__device__ __forceinline__ bool chroma_job(const svthip_warp_pu_desc& d, const WarpArgs& A, uint4& job)
{
    int r, c;
    clamp_mv_to_umv_border(d.mv[0], d.mv[1], d.mb_to_left_edge, d.mb_to_right_edge, d.mb_to_top_edge, d.mb_to_bottom_edge, chroma_side(A.bw),
                           chroma_side(A.bh), 1, r, c);
    const int64_t so = ((int64_t)chroma_origin(d.pu_origin_y) + (r >> 4)) * A.rcs + chroma_origin(d.pu_origin_x) + (c >> 4) + A.kc;
    const uint32_t cdst = (uint32_t)chroma_origin(d.dst_origin_y) * A.dcs + (uint32_t)chroma_origin(d.dst_origin_x);
    job = uni_job((uint32_t)so, cdst, c & 15, r & 15, 0, 0);  // interp_filters = 0
    return offset_in_range(so);
}

// one thread per PU; the list length sits in the 16 bytes in front of the jobs, one atomic per wave
__global__ void __launch_bounds__(256) warp_chroma_expand_kernel(const svthip_warp_pu_desc* __restrict__ desc, uint32_t n_pu, WarpArgs A,
                                                                 uint4* __restrict__ list)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    bool want = false;
    uint4 job = uint4{0u, 0u, 0u, 0u};
    if (i < n_pu) {
        const svthip_warp_pu_desc d = desc[i];
        want = d.has_uv && model_valid(d) && chroma_job(d, A, job);
    }
    const uint64_t mask = __ballot(want);
    if (!mask) return;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    uint32_t base = 0;
    if ((threadIdx.x & 63) == (uint32_t)__builtin_ctzll(mask)) base = atomicAdd(reinterpret_cast<uint32_t*>(list), (uint32_t)__popcll(mask));
    base = __builtin_amdgcn_readlane(base, __builtin_ctzll(mask));
    if (want) list[1 + base + below] = job;
}

__device__ __forceinline__ int tap(uint32_t lo, uint32_t hi, int m) { return (int)(int8_t)((m < 4 ? lo : hi) >> (8 * (m & 3))); }

template <bool HBD>
__global__ void __launch_bounds__(256) warp_kernel(const svthip_warp_pu_desc* __restrict__ desc, uint32_t n_pu, WarpArgs A, uint32_t* __restrict__ refused)
{
    __shared__ uint32_t filt[193][2];
    __shared__ uint16_t tmp[4][15 * 8];
    for (int i = threadIdx.x; i < 193 * 2; i += 256) (&filt[0][0])[i] = (&kWarpFilter[0][0])[i];
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int nbx = A.bw >> 3, nby = (A.bw >> 3) * (A.bh >> 3);
    const int ncx = A.bw >> 4, ncb = A.warp_chroma ? (A.bw >> 4) * (A.bh >> 4) : 0;
    const uint32_t per_pu = (uint32_t)(nby + 2 * ncb);
    const uint64_t n_units = (uint64_t)n_pu * per_pu;
    const int bd = HBD ? A.bd : 8;
    const int pix_max = (1 << bd) - 1;

#pragma unroll 1
    for (int it = 0; it < kBlocksPerWave; it++) {
        const uint64_t unit = (uint64_t)blockIdx.x * kBlocksPerGroup + (uint32_t)(it * 4 + wave);
        if (unit >= n_units) break;
        const uint32_t pu = (uint32_t)(unit / per_pu);
        int r = (int)(unit - (uint64_t)pu * per_pu);
        const svthip_warp_pu_desc d = desc[pu];
        bool ok = model_valid(d);
        if (ok && d.has_uv && !A.warp_chroma) {
            uint4 job;
            ok = chroma_job(d, A, job);
        }
        if (!ok) {
            if (r == 0 && lane == 0) atomicAdd(refused, 1u);
            continue;
        }
        // plane of this block
        int ss = 0, bx, by;
        const uint8_t* ref = A.ry;
        uint8_t* dst = A.dy;
        uint32_t rs = A.rys, ds = A.dys;
        if (r < nby) {
            by = r / nbx;
            bx = r - by * nbx;
        } else {
            if (!d.has_uv) continue;
            r -= nby;
            const bool cr = r >= ncb;
            if (cr) r -= ncb;
            ss = 1;
            by = r / ncx;
            bx = r - by * ncx;
            ref = cr ? A.rcr : A.rcb;
            dst = cr ? A.dcr : A.dcb;
            rs = A.rcs;
            ds = A.dcs;
        }
        const int width = A.pic_w >> ss, height = A.pic_h >> ss;
        // the block centre through the model (warp_plane :806-809: ROTZOOM takes mat[4], mat[5] from mat[3], mat[2]); 32-bit wrap-around
        const uint32_t m0 = (uint32_t)d.wmmat[0], m1 = (uint32_t)d.wmmat[1], m2 = (uint32_t)d.wmmat[2], m3 = (uint32_t)d.wmmat[3];
        const uint32_t m4 = d.wmtype == 2 ? 0u - m3 : (uint32_t)d.wmmat[4], m5 = d.wmtype == 2 ? m2 : (uint32_t)d.wmmat[5];
        const int j = (d.pu_origin_x >> ss) + 8 * bx, i = (d.pu_origin_y >> ss) + 8 * by;
        const uint32_t src_x = (uint32_t)(j + 4) << ss, src_y = (uint32_t)(i + 4) << ss;
        const int32_t dst_x = (int32_t)(m2 * src_x + m3 * src_y + m0), dst_y = (int32_t)(m4 * src_x + m5 * src_y + m1);
        const int32_t x4 = dst_x >> ss, y4 = dst_y >> ss;
        const int ix4 = x4 >> 16, iy4 = y4 >> 16;
        const int alpha = d.alpha, beta = d.beta, gamma = d.gamma, delta = d.delta;
        const int sx4 = ((x4 & 0xffff) + alpha * -4 + beta * -4) & ~63;
        const int sy4 = ((y4 & 0xffff) + gamma * -4 + delta * -4) & ~63;

        // ---- horizontal pass: result (k, l), k = 0..14 (source row iy4 + k - 7), l = 0..7 (samples ix4 + l - 7 .. ix4 + l) ----
        // fast path: the window and the aligned dwords around it (at most 3 bytes before, 3 after) lie inside the picture's rows
        const bool inside = !HBD && ix4 - 7 >= 4 && ix4 + 7 + 4 <= width - 1 && iy4 - 7 >= 0 && iy4 + 7 <= height - 1;
        const int l = lane & 7;
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            const int k = (lane >> 3) + 8 * pass;
            if (k < 15) {
                const int sx = sx4 + beta * (k - 3) + alpha * l;
                const int offs = min(max(((sx + 512) >> 10) + 64, 0), 192);
                const uint32_t flo = filt[offs][0], fhi = filt[offs][1];
                const int x0 = ix4 + l - 7;
                int sum;
                if (HBD) {
                    const int iy = min(max(iy4 + k - 7, 0), height - 1);
                    const uint16_t* row = reinterpret_cast<const uint16_t*>(ref) + (size_t)iy * rs;
                    sum = (1 << (bd + 6)) + 4;
#pragma unroll
                    for (int m = 0; m < 8; m++) sum += __mul24(tap(flo, fhi, m), (int)row[min(max(x0 + m, 0), width - 1)]);
                } else {
                    uint32_t lo, hi;
                    if (inside) {
                        const uint8_t* p = ref + (size_t)(iy4 + k - 7) * rs + x0;
                        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
                        const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
                        const uint32_t sh = (uint32_t)(a & 3u);
                        const uint32_t q0 = q[0], q1 = q[1], q2 = q[2];
                        lo = __builtin_amdgcn_alignbyte(q1, q0, sh);
                        hi = __builtin_amdgcn_alignbyte(q2, q1, sh);
                    } else {
                        const int iy = min(max(iy4 + k - 7, 0), height - 1);
                        const uint8_t* row = ref + (size_t)iy * rs;
                        lo = hi = 0;
#pragma unroll
                        for (int m = 0; m < 4; m++) {
                            lo |= (uint32_t)row[min(max(x0 + m, 0), width - 1)] << (8 * m);
                            hi |= (uint32_t)row[min(max(x0 + 4 + m, 0), width - 1)] << (8 * m);
                        }
                    }
                    // sum f p = sum f (p - 128) + 128 * 128; offset 1 << 14; rounding 4
                    sum = dot8(lo ^ 0x80808080u, hi ^ 0x80808080u, flo, fhi, (1 << 15) + 4);
                }
                tmp[wave][k * 8 + l] = (uint16_t)(sum >> 3);  // reduce_bits_horiz = 3 at 8 and 10 bits
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ---- vertical pass: output sample (k, l) of the block ----
        {
            const int k = lane >> 3;
            const int sy = sy4 + delta * k + gamma * l;
            const int offs = min(max(((sy + 512) >> 10) + 64, 0), 192);
            const uint32_t flo = filt[offs][0], fhi = filt[offs][1];
            int sum = (1 << (bd + 11)) + (1 << 10);  // offset_bits_vert = bd + 14 - 3, reduce_bits_vert = 11
#pragma unroll
            for (int m = 0; m < 8; m++) sum += __mul24(tap(flo, fhi, m), (int)tmp[wave][(k + m) * 8 + l]);
            int v = (sum >> 11) - (1 << (bd - 1)) - (1 << bd);
            v = min(max(v, 0), pix_max);
            const int dx0 = ss ? (d.dst_origin_x >> 3) << 2 : d.dst_origin_x, dy0 = ss ? (d.dst_origin_y >> 3) << 2 : d.dst_origin_y;
            const size_t o = (size_t)(dy0 + 8 * by + k) * ds + (size_t)(dx0 + 8 * bx + l);
            if (HBD) reinterpret_cast<uint16_t*>(dst)[o] = (uint16_t)v;
            else dst[o] = (uint8_t)v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

}  // namespace

bool warp_size_valid(int bw, int bh) { return convolve_size_valid(bw, bh) && bw >= 8 && bh >= 8; }

size_t warp_scratch_bytes(uint32_t n_pu) { return 16 + (size_t)n_pu * 16; }

hipError_t launch_warped_pred(const svthip_inter_planes& ref, const svthip_inter_planes& dst, int pic_w, int pic_h, const svthip_warp_pu_desc* desc,
                              uint32_t n_pu, int bw, int bh, int bd, void* scratch, uint32_t* refused, hipStream_t s)
{
    const int SB = bd > 8 ? 2 : 1;
    const int bwu = chroma_side(bw), bhu = chroma_side(bh);
    WarpArgs A;
    A.ry = static_cast<const uint8_t*>(ref.y); A.rcb = static_cast<const uint8_t*>(ref.cb); A.rcr = static_cast<const uint8_t*>(ref.cr);
    A.dy = static_cast<uint8_t*>(dst.y); A.dcb = static_cast<uint8_t*>(dst.cb); A.dcr = static_cast<uint8_t*>(dst.cr);
    A.rys = ref.y_stride; A.rcs = ref.c_stride; A.dys = dst.y_stride; A.dcs = dst.c_stride;
    A.pic_w = pic_w; A.pic_h = pic_h; A.bw = bw; A.bh = bh;
    A.warp_chroma = bw >= 16 && bh >= 16;
    A.bd = bd;
    A.kc = rebase_samples(bwu, bhu, ref.c_stride);
    hipError_t e;
    if (!A.warp_chroma) {
        uint4* list = static_cast<uint4*>(scratch);
        if ((e = hipMemsetAsync(list, 0, 16, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(warp_chroma_expand_kernel, dim3((n_pu + 255) / 256), dim3(256), 0, s, desc, n_pu, A, list);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        const uint8_t *cb = A.rcb - A.kc * SB, *cr = A.rcr - A.kc * SB;
        const ConvolveLaunch Lcb = {cb, ref.c_stride, nullptr, 0, dst.cb, dst.c_stride, list + 1, n_pu, bwu, bhu, bd, false, true};
        const ConvolveLaunch Lcr = {cr, ref.c_stride, nullptr, 0, dst.cr, dst.c_stride, list + 1, n_pu, bwu, bhu, bd, false, true};
        if ((e = launch_convolve_valu(Lcb, s)) != hipSuccess || (e = launch_convolve_valu(Lcr, s)) != hipSuccess) return e;
    }
    const uint64_t per_pu = (uint64_t)(bw >> 3) * (bh >> 3) + (A.warp_chroma ? 2 * (uint64_t)(bw >> 4) * (bh >> 4) : 0);
    const uint64_t groups = (n_pu * per_pu + kBlocksPerGroup - 1) / kBlocksPerGroup;
    if (groups > 0x7fffffffull) return hipErrorInvalidValue;
    if (bd > 8) hipLaunchKernelGGL(warp_kernel<true>, dim3((uint32_t)groups), dim3(256), 0, s, desc, n_pu, A, refused);
    else hipLaunchKernelGGL(warp_kernel<false>, dim3((uint32_t)groups), dim3(256), 0, s, desc, n_pu, A, refused);
    return hipGetLastError();
}

}  // namespace svthip
