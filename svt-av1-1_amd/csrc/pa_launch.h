// svt-av1-1_amd/csrc/pa_launch.h -- launch boundary of the picture-analysis family (pa_*.hip): what the C-ABI glue calls.
#pragma once
#include "svthip_internal.h"

namespace svthip {

// pa_planes.hip: the borders of the full-resolution plane and the 1/4 and 1/16 planes of n pool pictures (host array pics), in launches
// of up to SVTHIP_HME_MAX_JOBS pictures; generate_padding of one plane in place; svthip_me_cu_result -> the reference's MeCuResults_t
hipError_t launch_pa_derive_planes(uint8_t* pool, const svthip_pa_picture* pics, uint32_t n, bool do_quarter, bool do_sixteenth, hipStream_t s);
hipError_t launch_pad_plane(void* plane, uint32_t stride, int width, int height, int pad_w, int pad_h, int sample_bytes, hipStream_t s);
hipError_t launch_me_results_ref_layout(const svthip_me_cu_result* in, uint32_t n, svthip_me_cu_result_ref* out, hipStream_t s);

// pa_stats.hip: picture-analysis statistics -- block means / variances, homogeneity, histograms (kernels: pa_stats_kernels.h)
hipError_t launch_pa_block_stats(const uint8_t* pool, const svthip_pa_picture* pics, const int64_t* chroma_offsets, uint32_t n, uint32_t chroma_stride,
                                 int sub_precision, uint32_t n_sb, uint8_t* y_mean, uint16_t* variance, uint8_t* cb_mean, uint8_t* cr_mean, hipStream_t s);
hipError_t launch_pa_homogeneity(const uint16_t* variance, uint32_t width, uint32_t height, uint32_t n, uint32_t n_sb, uint64_t* var_of_var32x32,
                                 uint8_t* homogeneous, uint32_t* picture, hipStream_t s);
inline size_t pa_region_sum_bytes(size_t n) { return sizeof(uint32_t) * 16 * 3 * n; }  // SLOT_PA_REGION_SUMS: [n][16][3]
hipError_t launch_pa_histograms(const uint8_t* pool, const svthip_pa_picture* pics, const int64_t* chroma_offsets, uint32_t n, uint32_t chroma_stride,
                                uint32_t* histogram, uint32_t* region_intensity, uint32_t* average_intensity, uint32_t* region_sum, hipStream_t s);

// pa_noise.hip: input-picture noise detection and the weak denoising arms (kernels: pa_noise_kernels.h)
hipError_t launch_pa_noise_detect(const uint8_t* pool, const svthip_pa_picture* pics, uint32_t n, int sub_precision, uint32_t n_sb, uint8_t* denoised,
                                  uint32_t denoised_stride, uint64_t* sb_var, uint8_t* flat_noise, uint32_t* picture, hipStream_t s);
hipError_t launch_pa_denoise(uint8_t* pool, const svthip_pa_picture* pics, const int64_t* chroma_offsets, uint32_t n, uint32_t chroma_stride, uint32_t n_sb,
                             uint8_t* denoised, uint32_t denoised_stride, const uint8_t* flat_noise, const uint32_t* picture, hipStream_t s);

// pa_bitdepth.hip: the 10-bit picture forms over the three planes of n 4:2:0 pictures of w x h luma samples, one launch each (kernels:
// pa_bitdepth_kernels.h).  The svthip_planes arrays are host arrays of n entries.  outn == nullptr: the 8-bit plane alone.  `compressed`:
// inn is the SB-tiled compressed plane.  form: 0 = 8-bit planes, 1 + SVTHIP_SSE_SRC_* = 16-bit reconstruction against that source form;
// partial: pa_sse_partial_bytes(w, h, n) of scratch for the workgroups' sums (SLOT_PA_SSE_PARTIALS)
hipError_t launch_pa_unpack_10bit(const uint16_t* in16, const svthip_planes* in16_planes, uint8_t* out8, const svthip_planes* out8_planes, uint8_t* outn,
                                  const svthip_planes* outn_planes, uint32_t w, uint32_t h, uint32_t n, hipStream_t s);
hipError_t launch_pa_pack_10bit(const uint8_t* in8, const svthip_planes* in8_planes, const uint8_t* inn, const svthip_planes* inn_planes, bool compressed,
                                uint16_t* out16, const svthip_planes* out16_planes, uint32_t w, uint32_t h, uint32_t n, hipStream_t s);
size_t pa_sse_partial_bytes(uint32_t w, uint32_t h, uint32_t n);
hipError_t launch_pa_picture_sse(int form, const void* recon, const svthip_planes* recon_planes, const void* src, const svthip_planes* src_planes,
                                 const uint8_t* srcn, const svthip_planes* srcn_planes, uint32_t w, uint32_t h, uint32_t n, uint64_t* partial, uint64_t* sse,
                                 hipStream_t s);

}  // namespace svthip
