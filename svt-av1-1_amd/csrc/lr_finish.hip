// svt-av1-1_amd/csrc/lr_finish.hip -- the restoration decision on the device, host side: the launch of the kernel of lr_finish_kernels.h
// (rest_finish_search), and the whole restoration stage as one sequence of launches on one stream: Wiener search, self-guided search,
// decision, frame filter.  The contract is in include/svtav1_hip.h.  Not here: 12 bits, superres, more than one tile, force_restore_type.
#include "lr_launch.h"

#include "lr_finish_kernels.h"

namespace svthip {

hipError_t launch_rest_finish(const svthip_rest_finish_rates& rates, const uint32_t unit_base[4], int ps, int pe, const int64_t* wiener_sse,
                              const int16_t* taps, const int64_t* sgr_sse, const int32_t* sgrproj, uint8_t* unit_type, uint8_t* best_rtype,
                              svthip_rest_finish_result* result, uint32_t* refused, hipStream_t s)
{
    FinishArgs a;
    a.rates = rates;
    for (int p = 0; p < 4; p++) a.unit_base[p] = unit_base[p];
    a.plane_start = (uint32_t)ps;
    hipLaunchKernelGGL(rest_finish_kernel, dim3(pe - ps), dim3(kThreads), 0, s, a, wiener_sse, taps, sgr_sse, sgrproj, unit_type, best_rtype, result,
                       refused);
    return hipGetLastError();
}

// The workspace of the stage: the two searches' workspaces, then the tables the searches hand to the decision.
LrPickWorkspace lr_pick_workspace(uint32_t width, uint32_t height, const uint32_t unit_size[3])
{
    LrPickWorkspace w{};
    uint32_t base[4];
    const uint32_t n = lr_unit_geometry(width, height, unit_size, base, nullptr);
    WorkspaceLayout L;
    w.wiener = L.take(lr_workspace(n).total);
    w.sgr = L.take(sgr_workspace(width, height).total);
    w.wiener_sse = L.take((size_t)n * 2 * 8);
    w.sgr_sse = L.take((size_t)n * 8);
    w.n_trials = L.take((size_t)n * 4);
    w.pending = L.take(4);
    w.total = L.at;
    return w;
}

// restoration_seg_search + rest_finish_search + av1_loop_restoration_filter_frame.  The Wiener search runs its bound of trials, after which
// no unit is pending, so nothing here waits for the device.
hipError_t launch_lr_pick_filter(const svthip_lr_picture& pic, int bd, const svthip_rest_finish_rates& rates, void* work, void* const out[3],
                                 const uint32_t out_stride[3], uint8_t* unit_type, int16_t* taps, int32_t* sgrproj, svthip_rest_finish_result* result,
                                 uint32_t* refused, hipStream_t s)
{
    const LrPickWorkspace W = lr_pick_workspace(pic.width, pic.height, pic.unit_size);
    const WorkspaceView V{static_cast<uint8_t*>(work)};
    int64_t *wiener_sse = V.at<int64_t>(W.wiener_sse), *sgr_sse = V.at<int64_t>(W.sgr_sse);
    uint32_t base[4];
    lr_unit_geometry(pic.width, pic.height, pic.unit_size, base, nullptr);
    hipError_t e = launch_lr_search(pic, 0, 3, bd, 0, false, V.at<void>(W.wiener), wiener_sse, taps, V.at<int32_t>(W.n_trials), V.at<int32_t>(W.pending), s);
    if (e != hipSuccess) return e;
    e = launch_sgr_search(pic, 0, 3, bd, V.at<void>(W.sgr), sgrproj, sgr_sse, nullptr, s);
    if (e != hipSuccess) return e;
    e = launch_rest_finish(rates, base, 0, 3, wiener_sse, taps, sgr_sse, sgrproj, unit_type, nullptr, result, refused, s);
    if (e != hipSuccess) return e;
    return launch_lr_filter_frame(pic, out, out_stride, 0, 3, bd, unit_type, taps, sgrproj, refused, s);
}

}  // namespace svthip
