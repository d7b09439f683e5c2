// svt-av1-1_amd/csrc/fg_denoise.hip
//
// Film-grain Wiener denoising of a picture that is already in device memory, gfx950: the launches of fg_denoise_kernels.h.  Replaces
// aom_wiener_denoise_2d (Codec/noise_model.c:1363-1500) of the reference.  The filter stage is the tables and then four launches, one
// per half-overlapped pass in the reference's order, each a workgroup per block of all three planes; the dither stage is one launch of a
// workgroup per plane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svtav1_hip.h"
#include "fg_launch.h"
#include "fg_denoise_kernels.h"

namespace svthip {

static_assert(sizeof(FgdWork) <= 48 * 1024, "a block's work fits the LDS of a workgroup");
static_assert(FGD_LANES >= FGD_BLOCK && FGD_DITHER_ROWS == 64, "a lane per column of a block; a band of the dither is one wave");

FgDenoiseLayout fg_denoise_layout(uint32_t width, uint32_t height)
{
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    FgDenoiseLayout L;
    L.pitch = ((width + FGD_BLOCK - 1) / FGD_BLOCK + 2) * FGD_BLOCK;
    L.plane_floats = (size_t)L.pitch * (((height + FGD_BLOCK - 1) / FGD_BLOCK + 2) * FGD_BLOCK);
    L.err_rows = al(sizeof(double) * (FGD_TABLES_LUMA + FGD_TABLES_CHROMA));
    L.planes = L.err_rows + al(sizeof(float) * 3 * (size_t)width);
    L.total = L.planes + sizeof(float) * 3 * L.plane_floats;
    return L;
}

hipError_t launch_film_grain_wiener_filter(int bit_depth, const void* const data[3], const uint32_t stride[3], uint32_t width, uint32_t height,
                                           const float* const noise_psd[3], float* planes, double* tables, hipStream_t s)
{
    const FgDenoiseLayout L = fg_denoise_layout(width, height);
    FgdPicture P;
    for (int c = 0; c < 3; c++) P.data[c] = data[c], P.stride[c] = stride[c], P.result[c] = planes + c * L.plane_floats, P.psd[c] = noise_psd[c];
    P.w = (int32_t)width, P.h = (int32_t)height, P.bit_depth = bit_depth, P.pitch = (int32_t)L.pitch, P.tables = tables;
    P.nbw = (P.w + FGD_BLOCK - 1) / FGD_BLOCK, P.nbh = (P.h + FGD_BLOCK - 1) / FGD_BLOCK;
    hipLaunchKernelGGL(fgd_tables_kernel, dim3(2), dim3(FGM_LANES), 0, s, tables);
    const dim3 grid((P.nbw + 1) * (P.nbh + 1), 3);
    for (int pass = 0; pass < 4; pass++) {   // offsy outside, offsx inside (:1431-1434)
        if (bit_depth == 8)
            hipLaunchKernelGGL(fgd_filter_pass_kernel<uint8_t>, grid, dim3(FGD_LANES), 0, s, P, pass & 1, pass >> 1);
        else
            hipLaunchKernelGGL(fgd_filter_pass_kernel<uint16_t>, grid, dim3(FGD_LANES), 0, s, P, pass & 1, pass >> 1);
    }
    return hipGetLastError();
}

hipError_t launch_film_grain_dither(int bit_depth, const float* planes, void* const denoised[3], const uint32_t stride[3], uint32_t width, uint32_t height,
                                    float* err_rows, hipStream_t s)
{
    const FgDenoiseLayout L = fg_denoise_layout(width, height);
    FgdDither D;
    for (int c = 0; c < 3; c++) D.result[c] = planes + c * L.plane_floats, D.out[c] = denoised[c], D.stride[c] = stride[c], D.err_row[c] = err_rows + c * (size_t)width;
    D.w = (int32_t)width, D.h = (int32_t)height, D.bit_depth = bit_depth, D.pitch = (int32_t)L.pitch;
    if (bit_depth == 8)
        hipLaunchKernelGGL(fgd_dither_kernel<uint8_t>, dim3(3), dim3(FGD_DITHER_ROWS), 0, s, D);
    else
        hipLaunchKernelGGL(fgd_dither_kernel<uint16_t>, dim3(3), dim3(FGD_DITHER_ROWS), 0, s, D);
    return hipGetLastError();
}

}  // namespace svthip
