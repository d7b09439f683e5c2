// svt-av1-1_amd/csrc/pa_stats_kernels.h
//
// Picture-analysis statistics on the device, gfx950: the kernels of pa_stats.hip and the arithmetic they share with the host test
// (tests/host_kernels/pa_stats_host.cpp compiles this header with g++ and calls the __device__ functions below on plain arrays).
// Replaces (paths under Source/Lib of the reference; all of GatheringPictureStatistics, Codec/EbPictureAnalysisProcess.c:4742-4796,
// except what the header lists as out of scope):
//   ComputeBlockMeanComputeVariance                       Codec/EbPictureAnalysisProcess.c:1986-3005
//   ComputeChromaBlockMean / ZeroOutChromaBlockMean       :1626-1979
//   ComputePictureSpatialStatistics (SB loop, average)    :4633-4672
//   DetermineHomogeneousRegionInPicture                   :4491-4607
//   CalculateHistogram                                    :131-155
//   SubSampleLuma/ChromaGeneratePixelIntensityHistogramBins   :4129-4267
//   CalculateInputAverageIntensity (SCD_MODE_1 arm)       :4728-4732
//   ComputeMean8x8 / ComputeMeanOfSquaredValues8x8 / ComputeSubMean8x8 / ComputeSubdMeanOfSquaredValues8x8
//                                                         ASM_SSE2/EbComputeMean_Intrinsic_SSE2.c:9-146
//
// Fixed point as the reference: a mean is 8.8 (MEAN_PRECISION), a mean of squares 16.16 (VARIANCE_PRECISION).  An 8x8 leaf is
// sum << 2 and sumsq << 10 (all 8 rows) or, in the sub-sampled precision, sum << 3 and sumsq << 11 of rows 0, 2, 4, 6; both fit 32
// bits (64 * 255 << 2 = 65280, 64 * 255^2 << 10 = 4261478400 < 2^32).  Every level above is (a + b + c + d) >> 2 of its four
// children, means and means of squares separately, and that truncation is part of the result.  The tables are kept in the
// ME_TIER_ZERO_PU order the outputs have: [0] 64x64, [1..4] 32x32, [5..20] 16x16, [21..84] 8x8, each level in raster order.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/svtav1_hip.h"

namespace svthip {

// ------------------------------------------------------------------------------------------------ geometry

// first table entry of a level: 0 -> 0 (64x64), 1 -> 1 (32x32), 2 -> 5 (16x16), 3 -> 21 (8x8)
__device__ __forceinline__ int pa_level_first(int level) { return ((1 << (2 * level)) - 1) / 3; }

// table index of the top-left child of node k (raster) of `level`; the other three are + 1, + child_dim, + child_dim + 1
__device__ __forceinline__ int pa_first_child(int level, int k, int* child_dim)
{
    const int dim = 1 << level;
    *child_dim = 2 * dim;
    return pa_level_first(level + 1) + 2 * (k / dim) * 2 * dim + 2 * (k % dim);
}

// SB `sb` (raster) of a width x height picture: its origin, and whether all of it lies inside the picture (is_complete_sb)
__device__ __forceinline__ bool pa_sb_origin(uint32_t width, uint32_t height, uint32_t sb, uint32_t* x0, uint32_t* y0)
{
    const uint32_t nx = (width + 63u) >> 6;
    *x0 = (sb % nx) << 6;
    *y0 = (sb / nx) << 6;
    return *x0 + 64u <= width && *y0 + 64u <= height;
}

// One histogram region of one plane.  Luma (plane 0) is read from the 1/16 plane, every sample; chroma from the full-size chroma
// plane, every 4th column of every 4th row, in a region computed from the LUMA dimensions and halved.  (x0, y0), w, h are in samples
// of the plane read; the samples visited are (x0 + 4^(plane>0) i, y0 + ... j) for i < cols, j < rows.
struct PaHistRegion {
    uint32_t x0, y0, cols, rows, step;
    uint32_t round, div;  // region intensity = (uint8_t)((sum' + round) / div), sum' = sum (luma) or sum << 4 (chroma)
};
__device__ __forceinline__ PaHistRegion pa_hist_region(uint32_t width, uint32_t height, int plane, uint32_t rx, uint32_t ry)
{
    const uint32_t pw = plane ? width : width >> 2, ph = plane ? height : height >> 2;  // the reference's inputPicturePtr->width / height
    const uint32_t rw = pw / 4u, rh = ph / 4u;
    const uint32_t fw = rw + (rx == 3u ? pw - 4u * rw : 0u), fh = rh + (ry == 3u ? ph - 4u * rh : 0u);
    const uint32_t area = fw * fh;
    PaHistRegion r;
    if (plane == 0) {
        r.x0 = rx * rw, r.y0 = ry * rh, r.cols = fw, r.rows = fh, r.step = 1u;
        r.round = area >> 1, r.div = area;
    } else {
        r.x0 = (rx * rw) >> 1, r.y0 = (ry * rh) >> 1, r.step = 4u;
        r.cols = ((fw >> 1) + 3u) >> 2, r.rows = ((fh >> 1) + 3u) >> 2;
        r.round = area >> 3, r.div = area >> 2;
    }
    return r;
}

// ------------------------------------------------------------------------------------------------ leaves

// 8 samples of a row as two dwords.  ALIGNED: the row starts on a dword boundary (every luma row: offsets, strides and the 68-sample
// border are multiples of 4).  Otherwise, on the device, the row may start at any byte: the aligned dwords it touches are read and
// shifted together (v_alignbyte_b32), so such a row reads from the start of the dword of its first sample to the end of the dword of
// its last one, and nothing past that (a row that happens to be aligned reads its second dword twice instead of a third).
template <bool ALIGNED>
__device__ __forceinline__ void pa_load_row8(const uint8_t* p, uint32_t* lo, uint32_t* hi)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (ALIGNED) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        *lo = q[0], *hi = q[1];
        return;
    }
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
    const uint32_t d0 = q[0], d1 = q[1], d2 = q[sh ? 2 : 1];
    *lo = __builtin_amdgcn_alignbyte(d1, d0, sh);
    *hi = __builtin_amdgcn_alignbyte(d2, d1, sh);
#else
    memcpy(lo, p, 4);
    memcpy(hi, p + 4, 4);
#endif
}

// sum and sum of squares of 8 samples added to the running ones
__device__ __forceinline__ void pa_row8_sums(uint32_t lo, uint32_t hi, uint32_t* sum, uint32_t* sumsq)
{
#if defined(__HIP_DEVICE_COMPILE__)
    *sum = __builtin_amdgcn_sad_u8(hi, 0u, __builtin_amdgcn_sad_u8(lo, 0u, *sum));
    *sumsq = __builtin_amdgcn_udot4(hi, hi, __builtin_amdgcn_udot4(lo, lo, *sumsq, false), false);
#else
    for (int k = 0; k < 4; k++) {
        const uint32_t a = (lo >> (8 * k)) & 0xffu, b = (hi >> (8 * k)) & 0xffu;
        *sum += a + b;
        *sumsq += a * a + b * b;
    }
#endif
}

// One 8x8 leaf at `leaf` (rows `stride` apart) -> its fixed-point mean (8.8) and mean of squares (16.16); SUB: rows 0, 2, 4, 6 only.
// In two halves, so that a kernel can have the rows of two leaves on their way before it adds up the first.
template <int SUB, bool ALIGNED>
__device__ __forceinline__ void pa_leaf_load(const uint8_t* leaf, uint32_t stride, uint32_t lo[8], uint32_t hi[8])
{
#pragma unroll
    for (int r = 0; r < 8; r += 1 + SUB) pa_load_row8<ALIGNED>(leaf + (size_t)r * stride, &lo[r], &hi[r]);
}
template <int SUB>
__device__ __forceinline__ void pa_leaf_reduce(const uint32_t lo[8], const uint32_t hi[8], uint32_t* mean, uint32_t* mean_sq)
{
    uint32_t sum = 0, sumsq = 0;
#pragma unroll
    for (int r = 0; r < 8; r += 1 + SUB) pa_row8_sums(lo[r], hi[r], &sum, &sumsq);
    *mean = sum << (2 + SUB);
    *mean_sq = sumsq << (10 + SUB);
}
template <int SUB, bool ALIGNED>
__device__ __forceinline__ void pa_leaf(const uint8_t* leaf, uint32_t stride, uint32_t* mean, uint32_t* mean_sq)
{
    uint32_t lo[8], hi[8];
    pa_leaf_load<SUB, ALIGNED>(leaf, stride, lo, hi);
    pa_leaf_reduce<SUB>(lo, hi, mean, mean_sq);
}

// ------------------------------------------------------------------------------------------------ pyramid and outputs

// node k of `level` (0: 64x64, 1: 32x32, 2: 16x16) of a table in output order from its four children: (a + b + c + d) >> 2
__device__ __forceinline__ void pa_pyramid_node(uint32_t* table, int level, int k)
{
    int cd;
    const int c = pa_first_child(level, k, &cd);
    table[pa_level_first(level) + k] = (uint32_t)(((uint64_t)table[c] + table[c + 1] + table[c + cd] + table[c + cd + 1]) >> 2);
}

// The chroma tables have 21 entries, [0] 64x64, [1..4] 32x32, [5..20] the 8x8 chroma leaves ("16x16").  Their 64x64 mean counts the
// last 32x32 twice and the third not at all, as the reference (:1926-1927)
__device__ __forceinline__ void pa_chroma_top(uint32_t* table) { table[0] = (uint32_t)(((uint64_t)table[1] + table[2] + table[4] + table[4]) >> 2); }

__device__ __forceinline__ uint8_t pa_mean_out(uint32_t mean) { return (uint8_t)(mean >> 8); }
// unsigned 64-bit as the reference: mean * mean reaches 65280^2 = 4261478400, past what a signed 32-bit product holds
__device__ __forceinline__ uint16_t pa_variance_out(uint32_t mean, uint32_t mean_sq)
{
    return (uint16_t)(((uint64_t)mean_sq - (uint64_t)mean * (uint64_t)mean) >> 16);
}

// DetermineHomogeneousRegionInPicture for one SB from its 85 variances: the four 32x32-based variances of the 8x8 variances and
// whether the 64x64-based one stays at or below VAR_BASED_DETAIL_PRESERVATION_SELECTOR_THRSLHD (64 * 64).  An 8x8 variance is at most
// 127.5^2, so the reference's int products do not overflow and plain unsigned arithmetic restates them.
__device__ __forceinline__ uint8_t pa_sb_homogeneity(const uint16_t* variance, bool complete, uint64_t var_of_var32x32[4])
{
    if (!complete) {
        for (int q = 0; q < 4; q++) var_of_var32x32[q] = ~(uint64_t)0;
        return 1;
    }
    uint64_t sq_all = 0, v_all = 0;
    for (int q = 0; q < 4; q++) {
        uint64_t sq = 0, v = 0;
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                const uint64_t x = variance[21 + ((q >> 1) * 4 + r) * 8 + (q & 1) * 4 + c];
                sq += x * x;
                v += x;
            }
        sq_all += sq, v_all += v;
        sq >>= 4, v >>= 4;
        var_of_var32x32[q] = sq - v * v;
    }
    sq_all >>= 6, v_all >>= 6;
    return (sq_all - v_all * v_all) > 64u * 64u ? 0 : 1;
}

// picture[4] of svthip_pa_homogeneity_dev from the three sums over the SBs of a picture
__device__ __forceinline__ void pa_picture_flags(uint32_t total_variance, uint32_t very_low, uint32_t complete, uint32_t n_sb, uint32_t out[4])
{
    const uint32_t pct = very_low * 100u / complete;  // complete > 0: the entry refuses pictures smaller than one SB
    out[0] = (uint16_t)(total_variance / n_sb);
    out[1] = pct > 60u;  // PIC_LOW_VAR_PERCENTAGE_TH
    out[2] = pct > 80u;
    out[3] = complete;
}

// average_intensity of one plane from the sum over the 16 regions of (region sum << 4); width, height: luma
__device__ __forceinline__ uint32_t pa_average_intensity(uint64_t total, uint32_t width, uint32_t height, int plane)
{
    const uint64_t area = (uint64_t)width * height;
    return (uint8_t)(plane ? (total + (area >> 3)) / (area >> 2) : (total + (area >> 1)) / area);
}
__device__ __forceinline__ uint32_t pa_region_intensity(const PaHistRegion& r, int plane, uint32_t sum)
{
    return (uint8_t)(((uint64_t)(plane ? sum << 4 : sum) + r.round) / r.div);
}

// ------------------------------------------------------------------------------------------------ kernels
#ifdef __HIPCC__

// the pictures of one launch, by value: plane descriptors and the byte offsets in the pool of Cb and Cr sample (0, 0)
struct PaStatsJobTable {
    svthip_pa_picture pic[SVTHIP_HME_MAX_JOBS];
    int64_t chroma[SVTHIP_HME_MAX_JOBS][2];
};

// pa_noise_kernels.h takes the arithmetic above and the job table and leaves the kernels to pa_stats.hip, their one translation unit
#ifndef SVTHIP_PA_STATS_WITHOUT_KERNELS

// grid (n_sb, n pictures), one wave per SB.  Lane l owns luma leaf l (row l >> 3, column l & 7: 8 neighbouring lanes read one 64-byte
// row segment per load); lanes 0..31 also own a chroma leaf (Cb 0..15, Cr 16..31) of a complete SB.  The three levels above go
// through LDS: luma nodes on lanes 0.., chroma nodes on lanes 32.. in the same step.
template <int SUB>
__global__ void __launch_bounds__(64) pa_block_stats_kernel(const uint8_t* __restrict__ pool, PaStatsJobTable jobs, uint32_t chroma_stride,
                                                            uint8_t* __restrict__ y_mean, uint16_t* __restrict__ variance,
                                                            uint8_t* __restrict__ cb_mean, uint8_t* __restrict__ cr_mean)
{
    __shared__ uint32_t mean[85], mean_sq[85], cmean[2][21];
    const int lane = threadIdx.x;
    const uint32_t sb = blockIdx.x, n_sb = gridDim.x;
    const svthip_pa_picture P = jobs.pic[blockIdx.y];
    const int64_t cb_offset = jobs.chroma[blockIdx.y][0], cr_offset = jobs.chroma[blockIdx.y][1];  // scalar reads: no lane-indexed table
    uint32_t x0, y0;
    const bool complete = pa_sb_origin(P.width, P.height, sb, &x0, &y0);
    // an incomplete SB reads on into the replicated border: at most 56 samples of the 68 (width and height are multiples of 8)
    const uint8_t* leaf = pool + P.full_offset + (size_t)(68u + y0 + 8u * (lane >> 3)) * P.full_stride + 68u + x0 + 8u * (lane & 7);
    uint32_t lo[8], hi[8];
    pa_leaf_load<SUB, true>(leaf, P.full_stride, lo, hi);
    if (lane < 32) {
        uint32_t m = 0, unused;
        if (complete) {
            const int cl = lane & 15;
            const uint8_t* c = pool + (lane < 16 ? cb_offset : cr_offset) + (size_t)((y0 >> 1) + 8u * (cl >> 2)) * chroma_stride + (x0 >> 1) + 8u * (cl & 3);
            pa_leaf<SUB, false>(c, chroma_stride, &m, &unused);
        }
        cmean[lane >> 4][5 + (lane & 15)] = m;
    }
    pa_leaf_reduce<SUB>(lo, hi, &mean[21 + lane], &mean_sq[21 + lane]);
    __syncthreads();
    if (lane < 16) {
        pa_pyramid_node(mean, 2, lane);
        pa_pyramid_node(mean_sq, 2, lane);
    } else if (lane >= 32 && lane < 40) {
        pa_pyramid_node(cmean[(lane - 32) >> 2], 1, lane & 3);
    }
    __syncthreads();
    if (lane < 4) {
        pa_pyramid_node(mean, 1, lane);
        pa_pyramid_node(mean_sq, 1, lane);
    } else if (lane >= 32 && lane < 34) {
        pa_chroma_top(cmean[lane - 32]);
    }
    __syncthreads();
    if (lane == 0) {
        pa_pyramid_node(mean, 0, 0);
        pa_pyramid_node(mean_sq, 0, 0);
    }
    __syncthreads();
    const size_t o = (size_t)blockIdx.y * n_sb + sb;
    for (int i = lane; i < 85; i += 64) {
        y_mean[o * 85 + i] = pa_mean_out(mean[i]);
        variance[o * 85 + i] = pa_variance_out(mean[i], mean_sq[i]);
    }
    if (lane < 42) (lane < 21 ? cb_mean : cr_mean)[o * 21 + lane % 21] = pa_mean_out(cmean[lane / 21][lane % 21]);
}

// grid (n pictures): a lane per SB, the picture's three sums through LDS
__global__ void __launch_bounds__(256) pa_homogeneity_kernel(const uint16_t* __restrict__ variance, uint32_t width, uint32_t height, uint32_t n_sb,
                                                             uint64_t* __restrict__ var_of_var32x32, uint8_t* __restrict__ homogeneous,
                                                             uint32_t* __restrict__ picture)
{
    __shared__ uint32_t acc[3];  // sum of the 64x64 variances of ALL SBs; complete SBs below LCU_LOW_VAR_TH; complete SBs
    const size_t first = (size_t)blockIdx.x * n_sb;
    if (threadIdx.x < 3) acc[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t sb = threadIdx.x; sb < n_sb; sb += 256) {
        const uint16_t* v = variance + (first + sb) * 85;
        uint32_t x0, y0;
        const bool complete = pa_sb_origin(width, height, sb, &x0, &y0);
        uint64_t vov[4];
        homogeneous[first + sb] = pa_sb_homogeneity(v, complete, vov);
        for (int q = 0; q < 4; q++) var_of_var32x32[(first + sb) * 4 + q] = vov[q];
        atomicAdd(&acc[0], (uint32_t)v[0]);
        if (complete) {
            atomicAdd(&acc[2], 1u);
            if (v[0] < 5) atomicAdd(&acc[1], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t out[4];
        pa_picture_flags(acc[0], acc[1], acc[2], n_sb, out);
        for (int k = 0; k < 4; k++) picture[blockIdx.x * 4 + k] = out[k];
    }
}

// grid (16 regions, 3 planes, n pictures): a 256-bin histogram in LDS; the bins leave as (1 + count) << 4 (the reference starts every
// bin at 1 and scales by 16 afterwards).  region_sum [n][16][3] takes sum << 4 for pa_average_kernel.
__global__ void __launch_bounds__(256) pa_histogram_kernel(const uint8_t* __restrict__ pool, PaStatsJobTable jobs, uint32_t chroma_stride,
                                                           uint32_t* __restrict__ histogram, uint32_t* __restrict__ region_intensity,
                                                           uint32_t* __restrict__ region_sum)
{
    __shared__ uint32_t bins[256], total;
    const uint32_t rx = blockIdx.x >> 2, ry = blockIdx.x & 3u;
    const int plane = blockIdx.y;
    const svthip_pa_picture P = jobs.pic[blockIdx.z];
    const PaHistRegion R = pa_hist_region(P.width, P.height, plane, rx, ry);
    const uint32_t stride = plane ? chroma_stride : P.sixteenth_stride;
    const uint8_t* origin = plane ? pool + jobs.chroma[blockIdx.z][plane - 1] : pool + P.sixteenth_offset + (size_t)16 * stride + 16;
    bins[threadIdx.x] = 0;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    uint32_t sum = 0;
    for (uint32_t i = threadIdx.x; i < R.cols * R.rows; i += 256) {
        const uint32_t j = i / R.cols;
        const uint32_t v = origin[(size_t)(R.y0 + j * R.step) * stride + R.x0 + (i - j * R.cols) * R.step];
        atomicAdd(&bins[v], 1u);
        sum += v;
    }
    atomicAdd(&total, sum);
    __syncthreads();
    const size_t o = ((size_t)blockIdx.z * 16 + blockIdx.x) * 3 + plane;  // [picture][region x][region y][plane]
    histogram[o * 256 + threadIdx.x] = (1u + bins[threadIdx.x]) << 4;
    if (threadIdx.x == 0) {
        region_intensity[o] = pa_region_intensity(R, plane, total);
        region_sum[o] = total << 4;
    }
}

// grid (n pictures): lanes 0..2 add up the 16 region sums of their plane
__global__ void __launch_bounds__(64) pa_average_kernel(const uint32_t* __restrict__ region_sum, PaStatsJobTable jobs, uint32_t* __restrict__ average_intensity)
{
    if (threadIdx.x >= 3) return;
    uint64_t t = 0;
    for (int r = 0; r < 16; r++) t += region_sum[((size_t)blockIdx.x * 16 + r) * 3 + threadIdx.x];
    average_intensity[blockIdx.x * 3 + threadIdx.x] = pa_average_intensity(t, jobs.pic[blockIdx.x].width, jobs.pic[blockIdx.x].height, (int)threadIdx.x);
}

#endif  // SVTHIP_PA_STATS_WITHOUT_KERNELS
#endif  // __HIPCC__

}  // namespace svthip
