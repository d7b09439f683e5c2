// svt-av1-1_amd/csrc/pa_noise.hip
//
// Input-picture noise detection and denoising of pictures that are already in device memory, gfx950: the launches of pa_noise_kernels.h.
// Replaces FullSampleDenoise (Codec/EbPictureAnalysisProcess.c:3357-3410) of the reference in two entries: DetectInputPictureNoise (the
// weak luma filter, the noise and denoised variances of every complete SB, sb_flat_noise_array, pic_noise_class) in one read pass over
// the luma interior, and the weak arms of DenoiseInputPicture in place on the pool, the arm chosen on the device from what the first
// entry left.  Neither reads a border sample, so both run before svthip_pa_derive_planes_dev.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/svtav1_hip.h"
#include "pa_launch.h"
#include "pa_noise_kernels.h"

namespace svthip {

namespace {

PaStatsJobTable pa_noise_job_table(const svthip_pa_picture* pics, const int64_t* chroma_offsets, uint32_t n)
{
    PaStatsJobTable jt;
    memset(&jt, 0, sizeof(jt));
    for (uint32_t j = 0; j < n; j++) {
        jt.pic[j] = pics[j];
        if (chroma_offsets) jt.chroma[j][0] = chroma_offsets[2 * j], jt.chroma[j][1] = chroma_offsets[2 * j + 1];
    }
    return jt;
}

template <int SUB, bool WRITE>
void detect(const PaStatsJobTable& jt, const uint8_t* pool, uint32_t n, uint32_t n_sb, uint8_t* denoised, uint32_t denoised_stride, uint64_t* sb_var,
            uint8_t* flat_noise, hipStream_t s)
{
    hipLaunchKernelGGL((pa_noise_detect_kernel<SUB, WRITE>), dim3(n_sb, n), dim3(64), 0, s, pool, jt, denoised, denoised_stride, sb_var, flat_noise);
}

}  // namespace

hipError_t launch_pa_noise_detect(const uint8_t* pool, const svthip_pa_picture* pics, uint32_t n, int sub_precision, uint32_t n_sb, uint8_t* denoised,
                                  uint32_t denoised_stride, uint64_t* sb_var, uint8_t* flat_noise, uint32_t* picture, hipStream_t s)
{
    const PaStatsJobTable jt = pa_noise_job_table(pics, nullptr, n);
    if (denoised)
        (sub_precision ? detect<1, true> : detect<0, true>)(jt, pool, n, n_sb, denoised, denoised_stride, sb_var, flat_noise, s);
    else
        (sub_precision ? detect<1, false> : detect<0, false>)(jt, pool, n, n_sb, nullptr, 0, sb_var, flat_noise, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pa_noise_picture_kernel, dim3(n), dim3(256), 0, s, (const uint64_t*)sb_var, pics[0].width, pics[0].height, n_sb, picture);
    return hipGetLastError();
}

// Three launches on one stream: the luma of the SBs the arm names from `denoised` into the pool; then, with the luma gone from it,
// `denoised` takes the filtered chroma of whole-picture pictures; then that goes back into the pool.
hipError_t launch_pa_denoise(uint8_t* pool, const svthip_pa_picture* pics, const int64_t* chroma_offsets, uint32_t n, uint32_t chroma_stride, uint32_t n_sb,
                             uint8_t* denoised, uint32_t denoised_stride, const uint8_t* flat_noise, const uint32_t* picture, hipStream_t s)
{
    const PaStatsJobTable jt = pa_noise_job_table(pics, chroma_offsets, n);
    hipLaunchKernelGGL(pa_denoise_luma_kernel, dim3(n_sb, n), dim3(64), 0, s, pool, jt, (const uint8_t*)denoised, denoised_stride, flat_noise, picture);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid(pics[0].height / 2, 2, n);
    hipLaunchKernelGGL(pa_denoise_chroma_kernel<true>, grid, dim3(128), 0, s, pool, jt, chroma_stride, denoised, denoised_stride, picture);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pa_denoise_chroma_kernel<false>, grid, dim3(128), 0, s, pool, jt, chroma_stride, denoised, denoised_stride, picture);
    return hipGetLastError();
}

}  // namespace svthip
