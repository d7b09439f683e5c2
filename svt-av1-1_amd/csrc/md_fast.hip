// svt-av1-1_amd/csrc/md_fast.hip
//
// Mode decision's fast loop on predictions that are already in device memory, gfx950: the launches of md_fast_kernels.h.
// Replaces what the second loop of ProductPerformFastLoop (Codec/EbProductCodingLoop.c:1282-1459) does after each prediction -- the three
// SADs against the source picture and the fast cost -- in one launch per luma size, and its buffer replacement with PreModeDecision
// (Codec/EbModeDecision.c:393-471) in one launch over the blocks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svtav1_hip.h"
#include "md_launch.h"
#include "md_fast_kernels.h"

namespace svthip {

namespace {

template <int G>
hipError_t launch_cost(const MdFastArgs& A, hipStream_t s)
{
    constexpr uint64_t per_workgroup = 4u * (64u / G);
    hipLaunchKernelGGL(md_fast_cost_kernel<G>, dim3((uint32_t)((A.n + per_workgroup - 1u) / per_workgroup)), dim3(256), 0, s, A);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_md_fast_cost(const svthip_inter_planes& src, const svthip_inter_planes& pred, const svthip_md_fast_desc* desc, uint32_t n_cand,
                               uint32_t bwidth, uint32_t bheight, svthip_md_fast_result* result, hipStream_t s)
{
    const MdFastArgs A = md_fast_make_args(src, pred, desc, n_cand, bwidth, bheight, result);
    switch (md_fast_group_lanes(bwidth, bheight)) {
    case 4: return launch_cost<4>(A, s);
    case 8: return launch_cost<8>(A, s);
    case 16: return launch_cost<16>(A, s);
    case 32: return launch_cost<32>(A, s);
    default: return launch_cost<64>(A, s);
    }
}

hipError_t launch_md_fast_pick(const svthip_md_fast_result* result, const svthip_md_fast_desc* desc, uint32_t n_cand, const svthip_md_fast_group* group,
                               uint32_t n_groups, svthip_md_fast_pick* pick, uint32_t* refused, hipStream_t s)
{
    hipLaunchKernelGGL(md_fast_pick_kernel, dim3((uint32_t)(((uint64_t)n_groups + MD_FAST_PICK_THREADS - 1u) / MD_FAST_PICK_THREADS)), dim3(MD_FAST_PICK_THREADS), 0, s, result,
                       desc, n_cand, group, n_groups, pick, refused);
    return hipGetLastError();
}

}  // namespace svthip
