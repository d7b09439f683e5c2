// svt-av1-1_amd/csrc/lr_sgrproj.hip -- self-guided loop restoration on the device, host side: the workspace, the launches of the kernels
// of lr_sgrproj_kernels.h, the whole search, the SSE trial and the self-guided pass of the frame filter (lr_wiener.hip starts it).  The
// contract is in include/svtav1_hip.h.  Not here: rest_finish_search (lr_finish.hip), CDEF (cf_cdef.hip), 12 bits, superres, more than
// one tile.
#include "lr_launch.h"

#include "lr_sgrproj_kernels.h"

namespace svthip {

uint32_t sgr_walk_max_trials() { return kSgrWalkMaxTrials; }

// The workspace of the search: per (unit, set) job the sums, size, set, xq, start xqd, final xqd, error and trial count, sized for the
// most units a picture of this size can have (unit size 64 in every plane), then f0 / f1 of every set: per plane [16][2][rows][columns] int16.
SgrWorkspace sgr_workspace(uint32_t width, uint32_t height)
{
    SgrWorkspace w;
    WorkspaceLayout L;
    const size_t jobs = (size_t)3 * units_in((int)width, 64) * units_in((int)height, 64) * kSgrParams;
    w.sums = L.take(jobs * 5 * 8);
    w.err = L.take(jobs * 8);
    w.size = L.take(jobs * 4);
    w.ep = L.take(jobs * 4);
    w.ntr = L.take(jobs * 4);
    w.xq = L.take(jobs * 8);
    w.start = L.take(jobs * 8);
    w.fin = L.take(jobs * 8);
    for (int p = 0; p < 3; p++) w.f[p] = L.take((size_t)(width >> (p > 0)) * (height >> (p > 0)) * kSgrParams * 2 * sizeof(int16_t));
    w.total = L.at;
    return w;
}

// the self-guided unit filter over the planes: trial (sse) or frame filter (out)
template <bool WRITE>
static hipError_t sgr_filter(const svthip_lr_picture& pic, void* const out[3], const uint32_t out_stride[3], int ps, int pe, int bd, const int32_t* sgrproj,
                             const uint8_t* flag, int64_t* sse, uint32_t* refused, hipStream_t s)
{
    return by_bit_depth(bd, [&](auto t) {
        using T = typename decltype(t)::type;
        return launch_unit_filter<T, WRITE>(sgr_filter_kernel<T, WRITE>, sgr_filter_grid, pic, out, out_stride, ps, pe, bd, sse, s, sgrproj, flag,
                                            reinterpret_cast<unsigned long long*>(sse), refused);
    });
}

hipError_t launch_sgr_filter_frame(const svthip_lr_picture& pic, void* const out[3], const uint32_t out_stride[3], int ps, int pe, int bd,
                                   const uint8_t* unit_type, const int32_t* sgrproj, uint32_t* refused, hipStream_t s)
{
    return sgr_filter<true>(pic, out, out_stride, ps, pe, bd, sgrproj, unit_type, nullptr, refused, s);
}

hipError_t launch_sgr_trial(const svthip_lr_picture& pic, int ps, int pe, int bd, const int32_t* sgrproj, const uint8_t* skip, int64_t* sse, hipStream_t s)
{
    return sgr_filter<false>(pic, nullptr, nullptr, ps, pe, bd, sgrproj, skip, sse, nullptr, s);
}

hipError_t launch_sgr_plane(const svthip_lr_picture& pic, int p, int bd, int ep, int32_t* flt0, int32_t* flt1, uint32_t flt_stride, hipStream_t s)
{
    return by_bit_depth(bd, [&](auto t) {
        using T = typename decltype(t)::type;
        const PlaneGeom g = plane_geom(pic.width, pic.height, pic.unit_size, p);
        hipLaunchKernelGGL((sgr_box_kernel<T, false>), sgr_box_grid(g), dim3(kThreads), 0, s, plane_ptr<T>(pic.cdef[p]), pic.cdef_stride[p],
                           (const T*)nullptr, 0u, g, bd, ep, ep + 1, flt0, flt1, flt_stride, (int16_t*)nullptr, (unsigned long long*)nullptr);
        return hipGetLastError();
    });
}

hipError_t launch_sgr_solve(const int64_t* sums, const int32_t* size, const int32_t* ep, uint32_t n, int32_t* xq, int32_t* xqd, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sgr_solve_kernel, lane_grid(n), dim3(64), 0, s, sums, size, ep, n, xq, xqd);
    return hipGetLastError();
}

hipError_t launch_sgr_walk_table(const int64_t* tables, const int32_t* ep, const int32_t* start, uint32_t n, int32_t* xqd, int64_t* err, int32_t* n_trials,
                                 hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sgr_walk_table_kernel, lane_grid(n), dim3(64), 0, s, tables, ep, start, n, xqd, err, n_trials);
    return hipGetLastError();
}

// search_sgrproj_seg for the units of the planes: box filter and sums, solve, walk, pick, then the SSE of the picked filter in filter geometry
hipError_t launch_sgr_search(const svthip_lr_picture& pic, int ps, int pe, int bd, void* work, int32_t* sgrproj, int64_t* sse, svthip_sgrproj_detail* detail,
                             hipStream_t s)
{
    return by_bit_depth(bd, [&](auto t) {
        using T = typename decltype(t)::type;
        const SgrWorkspace W = sgr_workspace(pic.width, pic.height);
        const WorkspaceView V{static_cast<uint8_t*>(work)};
        int64_t *sums = V.at<int64_t>(W.sums), *err = V.at<int64_t>(W.err);
        int32_t *size = V.at<int32_t>(W.size), *ep = V.at<int32_t>(W.ep), *ntr = V.at<int32_t>(W.ntr);
        int32_t *xq = V.at<int32_t>(W.xq), *start = V.at<int32_t>(W.start), *fin = V.at<int32_t>(W.fin);
        for (int p = ps; p < pe; p++) {
            const PlaneGeom g = plane_geom(pic.width, pic.height, pic.unit_size, p);
            const uint32_t n = (uint32_t)(g.nx * g.ny), jobs = n * kSgrParams;
            const size_t job0 = (size_t)g.base * kSgrParams;
            int16_t* f16 = V.at<int16_t>(W.f[p]);
            hipLaunchKernelGGL(sgr_search_init_kernel, lane_grid(jobs), dim3(64), 0, s, g, sums, size, ep);
            hipLaunchKernelGGL((sgr_box_kernel<T, true>), sgr_box_grid(g), dim3(kThreads), 0, s, plane_ptr<T>(pic.cdef[p]), pic.cdef_stride[p],
                               plane_ptr<T>(pic.source[p]), pic.source_stride[p], g, bd, 0, kSgrParams, (int32_t*)nullptr, (int32_t*)nullptr, 0u, f16,
                               reinterpret_cast<unsigned long long*>(sums));
            hipLaunchKernelGGL(sgr_solve_kernel, lane_grid(jobs), dim3(64), 0, s, sums + job0 * 5, size + job0, ep + job0, jobs, xq + job0 * 2,
                               start + job0 * 2);
            hipLaunchKernelGGL(sgr_walk_kernel<T>, sgr_walk_grid(g), dim3(kThreads), 0, s, plane_ptr<T>(pic.cdef[p]), pic.cdef_stride[p],
                               plane_ptr<T>(pic.source[p]), pic.source_stride[p], g, f16, start, fin, err, ntr);
            hipLaunchKernelGGL(sgr_pick_kernel, lane_grid(n), dim3(64), 0, s, sums, xq, start, fin, err, ntr, (uint32_t)g.base, (uint32_t)g.base + n, sgrproj,
                               detail);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        return launch_sgr_trial(pic, ps, pe, bd, sgrproj, nullptr, sse, s);
    });
}

}  // namespace svthip
