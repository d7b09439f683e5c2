// svt-av1-1_amd/csrc/lr_launch.h -- launch boundary of the loop-restoration family (lr_*.hip): what the C-ABI glue calls.
#pragma once
#include "svthip_internal.h"

namespace svthip {

// lr_wiener.hip: Wiener loop restoration -- the unit geometry, the statistics, the solve, the unit filter as SSE trial, the refinement walk
// step by step and as the whole search, and the frame filter of the three unit types (kernels: lr_wiener_kernels.h)
struct LrWorkspace {   // byte offsets into the caller's workspace, and its size
    size_t raw, M, H, sse_none, trial_sse, state, start_taps, avg, rejected, total;
};
LrWorkspace lr_workspace(uint32_t n_units);
uint32_t lr_unit_geometry(uint32_t width, uint32_t height, const uint32_t unit_size[3], uint32_t unit_base[4], int32_t* limits);
uint32_t lr_walk_max_trials(int win);
hipError_t launch_lr_stats(const svthip_lr_picture& pic, int plane_start, int plane_end, int bd, void* raw, int64_t* M, int64_t* H, int32_t* avg,
                           int64_t* sse_none, hipStream_t s);
hipError_t launch_lr_solve(const int64_t* M, const int64_t* H, uint32_t unit_begin, uint32_t unit_end, int win, int16_t* taps, int32_t* rejected,
                           hipStream_t s);
hipError_t launch_lr_trial(const svthip_lr_picture& pic, int plane_start, int plane_end, int bd, const void* taps, size_t taps_stride,
                           const uint8_t* skip, size_t skip_stride, int64_t* sse, hipStream_t s);
hipError_t launch_lr_filter_frame(const svthip_lr_picture& pic, void* const out[3], const uint32_t out_stride[3], int plane_start, int plane_end,
                                  int bd, const uint8_t* unit_type, const int16_t* taps, const int32_t* sgrproj, uint32_t* refused, hipStream_t s);
hipError_t launch_lr_walk_init(svthip_wiener_walk_state* state, const int16_t* taps, const int32_t* rejected, uint32_t unit_begin, uint32_t unit_end,
                               int win, hipStream_t s);
hipError_t launch_lr_walk_step(svthip_wiener_walk_state* state, const int64_t* trial_sse, uint32_t unit_begin, uint32_t unit_end, int32_t* pending,
                               hipStream_t s);
SVTHIP_LOCAL hipError_t launch_lr_search(const svthip_lr_picture& pic, int plane_start, int plane_end, int bd, uint32_t n_steps, bool resume,
                                         void* work, int64_t* sse, int16_t* taps, int32_t* n_trials, int32_t* pending, hipStream_t s);
// lr_sgrproj.hip: self-guided loop restoration -- the box filter over a plane, the solve, the walk on tables, the whole search, the unit
// filter as SSE trial and as the self-guided pass of launch_lr_filter_frame (kernels: lr_sgrproj_kernels.h)
struct SgrWorkspace {   // byte offsets into the caller's workspace, and its size
    size_t sums, err, size, ep, ntr, xq, start, fin, f[3], total;
};
SgrWorkspace sgr_workspace(uint32_t width, uint32_t height);
uint32_t sgr_walk_max_trials();
hipError_t launch_sgr_plane(const svthip_lr_picture& pic, int plane, int bd, int ep, int32_t* flt0, int32_t* flt1, uint32_t flt_stride, hipStream_t s);
hipError_t launch_sgr_solve(const int64_t* sums, const int32_t* size, const int32_t* ep, uint32_t n, int32_t* xq, int32_t* xqd, hipStream_t s);
hipError_t launch_sgr_walk_table(const int64_t* tables, const int32_t* ep, const int32_t* start, uint32_t n, int32_t* xqd, int64_t* err, int32_t* n_trials,
                                 hipStream_t s);
hipError_t launch_sgr_search(const svthip_lr_picture& pic, int plane_start, int plane_end, int bd, void* work, int32_t* sgrproj, int64_t* sse,
                             svthip_sgrproj_detail* detail, hipStream_t s);
hipError_t launch_sgr_trial(const svthip_lr_picture& pic, int plane_start, int plane_end, int bd, const int32_t* sgrproj, const uint8_t* skip, int64_t* sse,
                            hipStream_t s);
SVTHIP_LOCAL hipError_t launch_sgr_filter_frame(const svthip_lr_picture& pic, void* const out[3], const uint32_t out_stride[3], int plane_start,
                                                int plane_end, int bd, const uint8_t* unit_type, const int32_t* sgrproj, uint32_t* refused,
                                                hipStream_t s);
// lr_finish.hip: the restoration decision (rest_finish_search) -- the walks over the searches' tables, the frame type and the unit types of
// each plane; and the restoration stage as one sequence of the launches above and this one (kernel: lr_finish_kernels.h)
struct LrPickWorkspace {   // byte offsets into the caller's workspace, and its size
    size_t wiener, sgr, wiener_sse, sgr_sse, n_trials, pending, total;
};
SVTHIP_LOCAL LrPickWorkspace lr_pick_workspace(uint32_t width, uint32_t height, const uint32_t unit_size[3]);
SVTHIP_LOCAL hipError_t launch_rest_finish(const svthip_rest_finish_rates& rates, const uint32_t unit_base[4], int plane_start, int plane_end,
                                           const int64_t* wiener_sse, const int16_t* taps, const int64_t* sgr_sse, const int32_t* sgrproj,
                                           uint8_t* unit_type, uint8_t* best_rtype, svthip_rest_finish_result* result, uint32_t* refused,
                                           hipStream_t s);
SVTHIP_LOCAL hipError_t launch_lr_pick_filter(const svthip_lr_picture& pic, int bd, const svthip_rest_finish_rates& rates, void* work,
                                              void* const out[3], const uint32_t out_stride[3], uint8_t* unit_type, int16_t* taps, int32_t* sgrproj,
                                              svthip_rest_finish_result* result, uint32_t* refused, hipStream_t s);

}  // namespace svthip
