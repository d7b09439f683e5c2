// svt-av1-1_amd/csrc/me_fullpel209.hip -- stand-alone kernel of the 209-PU full-pel search (see me_fullpel209_impl.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "me_fullpel209_impl.h"
#include "me_launch.h"

namespace svthip {

constexpr int kFp209MinWaves = 3;  // workgroups per CU: 168 VGPRs, the top of that bracket (see the spill history in me_fullpel209_impl.h)

__global__ void __launch_bounds__(256, kFp209MinWaves) fullpel209_kernel(const uint8_t* __restrict__ src_plane, uint32_t src_stride,
                                                            const uint8_t* __restrict__ ref_plane, uint32_t ref_stride,
                                                            const int32_t* __restrict__ desc, uint32_t n_sb, uint32_t* __restrict__ out_sad,
                                                            uint32_t* __restrict__ out_mv)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t sb = xcd_item(blockIdx.x, n_sb);  // raster neighbours share an XCD's L2 (svthip_internal.h)
    if (sb >= n_sb) return;
    // wave-uniform choice of the search-loop form (me_fullpel209_impl.h): clipped windows at the picture's left / right edge take the general one
    if ((desc[6 * sb + 4] & 15) == 0) fullpel209_sb<true>(src_plane, src_stride, ref_plane, ref_stride, desc + 6 * sb, sb, out_sad, out_mv, smem);
    else fullpel209_sb<false>(src_plane, src_stride, ref_plane, ref_stride, desc + 6 * sb, sb, out_sad, out_mv, smem);
}

hipError_t launch_fullpel209(const uint8_t* src, uint32_t src_stride, const uint8_t* ref, uint32_t ref_stride, const svthip_fullpel_desc* desc,
                             uint32_t n_sb, uint32_t max_sh, uint32_t* out_sad, uint32_t* out_mv, hipStream_t s)
{
    const size_t lds = (size_t)kFp209Fixed + (size_t)(max_sh + 63) * SVTHIP_FULLPEL_LDS_PITCH;
    hipLaunchKernelGGL(fullpel209_kernel, dim3(xcd_grid(n_sb)), dim3(256), lds, s, src, src_stride, ref, ref_stride,
                       reinterpret_cast<const int32_t*>(desc), n_sb, out_sad, out_mv);
    return hipGetLastError();
}

hipError_t fullpel209_raise_dynamic_lds() { return raise_dynamic_lds({reinterpret_cast<const void*>(fullpel209_kernel)}); }

}  // namespace svthip
