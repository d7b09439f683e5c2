// svt-av1-1_amd/csrc/ma_stats.hip
//
// Motion-analysis statistics of pictures whose planes, ME results and OIS candidates are already in device memory, gfx950: the launches
// of ma_stats_kernels.h.  Replaces what the reference's ME process, initial rate control and source-based operations derive from those
// tables and from two more passes over picture samples: ComputeDecimatedZzSad (Codec/EbMotionEstimationProcess.c:219-348), CalculateAcEnergy
// (Codec/EbSourceBasedOperationsProcess.c:347-408), the distortion histograms (Codec/EbMotionEstimationProcess.c:607-725),
// MeBasedGlobalMotionDetection (Codec/EbInitialRateControlProcess.c:253-406, 467-483) and the per-SB flags of DeriveSimilarCollocatedFlag,
// FailingMotionLcu and DetectUncoveredLcu (Codec/EbInitialRateControlProcess.c:1286-1329, Codec/EbSourceBasedOperationsProcess.c:214-341).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/svtav1_hip.h"
#include "ma_launch.h"
#include "ma_stats_kernels.h"

namespace svthip {

namespace {

MaSignalTable ma_signal_table(const svthip_ma_picture_params* params, uint32_t n)
{
    MaSignalTable t;
    memset(&t, 0, sizeof(t));
    for (uint32_t j = 0; j < n; j++) {
        t.pic[j] = {params[j].slice_is_intra, params[j].temporal_layer_index, params[j].hierarchical_levels, params[j].is_used_as_reference_flag,
                    params[j].intensity_transition_flag};
        t.ref_index[j] = params[j].ref_index;
    }
    return t;
}

MaPictureTable ma_picture_table(const svthip_pa_picture* cur, const svthip_pa_picture* prev, uint32_t n)
{
    MaPictureTable t;
    memset(&t, 0, sizeof(t));
    for (uint32_t j = 0; j < n; j++) {
        t.cur[j] = cur[j];
        if (prev) t.prev[j] = prev[j];
    }
    return t;
}

dim3 ma_sample_grid(uint32_t n_sb, uint32_t n) { return dim3((n_sb + SVTHIP_MA_SBS_PER_GROUP - 1) / SVTHIP_MA_SBS_PER_GROUP, n); }

}  // namespace

hipError_t launch_ma_zz_sad(const uint8_t* pool, const svthip_pa_picture* cur, const svthip_pa_picture* prev, uint32_t n, uint32_t n_sb, uint32_t* sad,
                            uint8_t* zz_cost, uint8_t* non_moving_index, hipStream_t s)
{
    hipLaunchKernelGGL(ma_zz_sad_kernel, ma_sample_grid(n_sb, n), dim3(64 * SVTHIP_MA_SBS_PER_GROUP), 0, s, pool, ma_picture_table(cur, prev, n), n_sb, sad,
                       zz_cost, non_moving_index);
    return hipGetLastError();
}

hipError_t launch_ma_ac_energy(const uint8_t* pool, const svthip_pa_picture* pics, const svthip_ma_picture_params* params, uint32_t n, uint32_t n_sb,
                               const uint8_t* y_mean, uint64_t* energy, uint64_t* mean, hipStream_t s)
{
    hipLaunchKernelGGL(ma_ac_energy_kernel, ma_sample_grid(n_sb, n), dim3(64 * SVTHIP_MA_SBS_PER_GROUP), 0, s, pool, ma_picture_table(pics, nullptr, n),
                       ma_signal_table(params, n), n_sb, y_mean, energy, mean);
    return hipGetLastError();
}

hipError_t launch_ma_distortion_stats(const svthip_me_cu_result* me, uint32_t pu_stride, const uint32_t* cand, uint32_t w, uint32_t h,
                                      const svthip_ma_picture_params* params, uint32_t n, uint32_t n_sb, uint32_t* rc_me_distortion, uint32_t* inter_index,
                                      uint32_t* intra_index, uint32_t* hist, uint32_t* full_sb_count, hipStream_t s)
{
    hipLaunchKernelGGL(ma_distortion_stats_kernel, dim3(n), dim3(256), 0, s, me, pu_stride, cand, w, h, n_sb, ma_signal_table(params, n), rc_me_distortion,
                       inter_index, intra_index, hist, full_sb_count);
    return hipGetLastError();
}

hipError_t launch_ma_global_motion(const svthip_me_cu_result* me, uint32_t pu_stride, uint32_t w, uint32_t h, const svthip_ma_picture_params* params,
                                   uint32_t n, uint32_t n_sb, int32_t* out, hipStream_t s)
{
    hipLaunchKernelGGL(ma_global_motion_kernel, dim3(n), dim3(256), 0, s, me, pu_stride, w, h, n_sb, ma_signal_table(params, n), out);
    return hipGetLastError();
}

hipError_t launch_ma_sb_flags(const uint8_t* y_mean, const uint16_t* variance, const uint8_t* ref_mean, const uint16_t* ref_var, uint32_t ref_stride,
                              const svthip_me_cu_result* me, uint32_t pu_stride, const uint32_t* cand, uint32_t w, uint32_t h,
                              const svthip_ma_picture_params* params, uint32_t n, uint32_t n_sb, uint8_t* flags, hipStream_t s)
{
    hipLaunchKernelGGL(ma_sb_flags_kernel, dim3((n_sb + 255) / 256, n), dim3(256), 0, s, y_mean, variance, ref_mean, ref_var, ref_stride, me, pu_stride, cand, w,
                       h, n_sb, ma_signal_table(params, n), flags);
    return hipGetLastError();
}

}  // namespace svthip
