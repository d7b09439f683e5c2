// svt-av1-1_amd/csrc/fg_grain.hip
//
// AV1 film-grain synthesis of a reconstructed picture that is already in device memory, gfx950: the launches of fg_grain_kernels.h.
// Replaces av1_add_film_grain / av1_add_film_grain_run (Codec/EbEncDecProcess.c:2001-2069, Codec/grainSynthesis.c:995-1382) of the
// reference in two launches: one workgroup builds the three grain templates and the three scaling tables, then one pass reads the source
// planes and writes the destination planes, every sample once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/svtav1_hip.h"
#include "fg_launch.h"
#include "fg_grain_kernels.h"

namespace svthip {

static_assert(FG_TAB_INT16 * sizeof(int16_t) == SVTHIP_FILM_GRAIN_TABLES_BYTES, "the table block of the header");
static_assert(FG_LUMA_H == SVTHIP_FILM_GRAIN_LUMA_H && FG_LUMA_W == SVTHIP_FILM_GRAIN_LUMA_W && FG_CHROMA_H == SVTHIP_FILM_GRAIN_CHROMA_H &&
                  FG_CHROMA_W == SVTHIP_FILM_GRAIN_CHROMA_W, "the template sizes of the header");

hipError_t launch_film_grain_tables(const svthip_film_grain_params& params, int bit_depth, int16_t* tables, hipStream_t s)
{
    const FgParams P = fg_narrow(params, bit_depth);
    switch (P.lag) {
    case 0: hipLaunchKernelGGL(fg_tables_kernel<0>, dim3(1), dim3(FG_TABLES_THREADS), 0, s, P, tables); break;
    case 1: hipLaunchKernelGGL(fg_tables_kernel<1>, dim3(1), dim3(FG_TABLES_THREADS), 0, s, P, tables); break;
    case 2: hipLaunchKernelGGL(fg_tables_kernel<2>, dim3(1), dim3(FG_TABLES_THREADS), 0, s, P, tables); break;
    default: hipLaunchKernelGGL(fg_tables_kernel<3>, dim3(1), dim3(FG_TABLES_THREADS), 0, s, P, tables); break;
    }
    return hipGetLastError();
}

hipError_t launch_film_grain_frame(const svthip_film_grain_params& params, int bit_depth, const void* const src[3], const uint32_t src_stride[3],
                                   void* const dst[3], const uint32_t dst_stride[3], uint32_t width, uint32_t height, const int16_t* tables, hipStream_t s)
{
    const FgFrame f = fg_make_frame(fg_narrow(params, bit_depth), src, src_stride, dst, dst_stride, width, height, tables);
    const dim3 grid((width + 255) / 256, (height + 15) / 16);
    if (bit_depth == 8)
        hipLaunchKernelGGL(fg_frame_kernel<uint8_t>, grid, dim3(256), 0, s, f);
    else
        hipLaunchKernelGGL(fg_frame_kernel<uint16_t>, grid, dim3(256), 0, s, f);
    return hipGetLastError();
}

}  // namespace svthip
