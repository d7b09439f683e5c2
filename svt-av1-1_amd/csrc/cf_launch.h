// svt-av1-1_amd/csrc/cf_launch.h -- launch boundary of the CDEF family (cf_cdef.hip): what the C-ABI glue calls.
#pragma once
#include "svthip_internal.h"

namespace svthip {

// cf_cdef.hip: CDEF -- the strength search over all filter blocks, the strength pick, the frame filter, dist_8x8 on block pairs
// (kernels: cf_cdef_kernels.h)
double cdef_lambda(int base_qindex, int bd);
hipError_t launch_cdef_search_mse(const svthip_cdef_picture& pic, int base_qindex, int bd, uint64_t* mse, uint8_t* counted, hipStream_t s);
hipError_t launch_cdef_pick(const uint64_t* mse, const uint8_t* counted, uint32_t nfb, int base_qindex, int bd, svthip_cdef_result* result,
                            int8_t* fb_strength, hipStream_t s);
// the same for pictures whose grid has 128-wide blocks: the search per 64x64 quadrant into `work` (cdef_search128_workspace_bytes), then the merge
size_t cdef_search128_workspace_bytes(uint32_t width, uint32_t height);
hipError_t launch_cdef_search_mse128(const svthip_cdef_picture& pic, int base_qindex, int bd, const svthip_lf_mi* mi, uint32_t mi_stride, uint64_t* work,
                                     uint64_t* mse, uint8_t* counted, hipStream_t s);
hipError_t launch_cdef_pick128(const uint64_t* mse, const uint8_t* counted, uint32_t nhfb, uint32_t nvfb, int base_qindex, int bd, const svthip_lf_mi* mi,
                               uint32_t mi_stride, svthip_cdef_result* result, int8_t* fb_strength, hipStream_t s);
hipError_t launch_cdef_frame(const svthip_cdef_picture& pic, const svthip_cdef_result* result, const int8_t* fb_strength, int plane_start,
                             int plane_end, int bd, hipStream_t s);
hipError_t launch_cdef_dist_8x8(const uint16_t* dst, const uint16_t* src, uint32_t n, int coeff_shift, uint64_t* out, hipStream_t s);

}  // namespace svthip
