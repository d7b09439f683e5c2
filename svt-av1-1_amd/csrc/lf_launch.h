// svt-av1-1_amd/csrc/lf_launch.h -- launch boundary of the deblocking family (lf_deblock.hip): what the C-ABI glue calls.
#pragma once
#include "svthip_internal.h"

namespace svthip {

// lf_deblock.hip: the deblocking filter of a picture, the SSE of every candidate level, and search_filter_level's walk over them
hipError_t launch_lf_frame(const svthip_lf_picture& pic, const svthip_lf_mi* mi, uint32_t mi_stride, const int32_t* levels, int sharpness,
                           int plane_start, int plane_end, int bd, hipStream_t s);
hipError_t launch_lf_sse_table(const svthip_lf_picture& pic, const svthip_lf_mi* mi, uint32_t mi_stride, int plane, int dir,
                               const int32_t* levels, int sharpness, int bd, uint64_t* sse, hipStream_t s);
hipError_t launch_lf_walk(const uint64_t* sse, int start_level, int only_4x4, int32_t* out0, int32_t* out1, uint64_t* visited, hipStream_t s);
hipError_t launch_lf_set_levels(int32_t* levels, const int32_t v[4], hipStream_t s);

}  // namespace svthip
