// svt-av1-1_amd/csrc/me_hme.hip
//
// Search-centre derivation of one reference list for a batch of superblocks, on gfx950:
// hme_mv_center_check, HmeLevel0/1/2 over the (up to) 2x2 search regions, best-region pick,
// CheckZeroZeroCenter and the full-pel search-window clipping -- the first half of the reference's
// MotionEstimateLcu (Source/Lib/Codec/EbMotionEstimation.c:6300-6738, :5882-6145, :4306-4758, :5466-5552).
// Output: one svthip_fullpel_desc per SB for fullpel85_kernel (me_fullpel.hip).
//
// Mapping: one 256-thread workgroup per SB, blockIdx.y = job (a current / reference picture pair of the launch's job
// table); wave r owns HME search region r (regions are independent through all three levels), lanes own search positions.
// Every level is the reference's SadLoopKernel (C_DEFAULT/EbComputeSAD_C.c:73-119): exhaustive SAD over a small window,
// strict '<' in raster order, which a (sad << k | raster index) wave-min reproduces exactly.  The block and a band of the
// window are staged in a per-wave LDS slice; SADs are v_qsad_pk_u16_u8 on LDS dwords (me_hme_impl.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "me_launch.h"
#include "me_sad_common.h"
#include "me_wave_reduce.h"
#include "pa_job_table.h"

namespace svthip {

namespace {
#include "me_hme_impl.h"
}  // namespace

// job table of one search-centre launch, passed by value in the kernel arguments (2.5 KB)
struct HmeJobTable {
    svthip_pa_picture cur[SVTHIP_HME_MAX_JOBS];
    svthip_pa_picture ref[SVTHIP_HME_MAX_JOBS];
};

__global__ void __launch_bounds__(256) hme_center_kernel(const uint8_t* __restrict__ pool, HmeJobTable jobs, svthip_me_params P,
                                                         uint32_t list_index, const svthip_sb_origin* __restrict__ sbs, uint32_t n_sb,
                                                         uint32_t n_jobs, const uint32_t* __restrict__ l0_best_mv64, uint32_t l0_mv_stride,
                                                         svthip_fullpel_desc* __restrict__ out_desc,
                                                         int16_t* __restrict__ out_center, int16_t* __restrict__ hme_state)
{
    __shared__ HmeShared sh;
    __shared__ __attribute__((aligned(16))) uint8_t hme_lds[4 * kHmeLdsPerWave];
    // one block per (job, SB), job = one current / reference picture pair; all per-SB inputs and outputs of job j live at [j * n_sb + i].
    // Blocks are mapped so that an XCD walks a contiguous range of (job, SB) pairs: raster neighbours share its L2 (svthip_internal.h).
    const uint32_t sbi = xcd_item(blockIdx.x, n_sb * n_jobs);
    if (sbi >= n_sb * n_jobs) return;
    const uint32_t job = sbi / n_sb, sb_local = sbi - job * n_sb;
    hme_center_sb(pool, jobs.cur[job], jobs.ref[job], P, list_index, sbs[sb_local].x, sbs[sb_local].y, sbi, l0_best_mv64,
                  l0_mv_stride, out_desc, out_center, hme_state, sh, hme_lds);
}

hipError_t launch_hme_centers(const uint8_t* pool, const svthip_pa_picture* cur, const svthip_pa_picture* ref, uint32_t n_jobs,
                              const svthip_me_params& P, uint32_t list_index, const svthip_sb_origin* sbs, uint32_t n_sb,
                              const uint32_t* l0_best_mv64, uint32_t l0_mv_stride, svthip_fullpel_desc* out_desc, int16_t* out_center,
                              int16_t* hme_state, hipStream_t s)
{
    const uint32_t mvs = l0_mv_stride ? l0_mv_stride : 1u;
    for (uint32_t j0 = 0; j0 < n_jobs; j0 += SVTHIP_HME_MAX_JOBS) {
        const uint32_t nj = jobs_in_chunk(n_jobs, j0);
        HmeJobTable jt;
        memset(&jt, 0, sizeof(jt));
        for (uint32_t j = 0; j < nj; j++) {
            jt.cur[j] = cur[j0 + j];
            jt.ref[j] = ref[j0 + j];
        }
        const size_t base = (size_t)j0 * n_sb;
        const uint32_t* mv64 = l0_best_mv64 ? l0_best_mv64 + base * mvs : nullptr;
        int16_t* cen = out_center ? out_center + 2 * base : nullptr;
        int16_t* st = hme_state ? hme_state + SVTHIP_HME_STATE_INT16 * base : nullptr;
        hipLaunchKernelGGL(hme_center_kernel, dim3(xcd_grid(n_sb * nj)), dim3(256), 0, s, pool, jt, P, list_index, sbs, n_sb, nj, mv64, mvs,
                           out_desc + base, cen, st);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

#ifdef SVTHIP_HME_STAMPS
// debug build only (tools/hme_stamps_probe.py): copy the phase stamps of the last launches to the host
extern "C" int svthip_debug_hme_stamps(void* host, size_t bytes)
{
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_hme_stamps), bytes < sizeof(g_hme_stamps) ? bytes : sizeof(g_hme_stamps));
}
extern "C" int svthip_debug_hme_loop_phases(unsigned long long* host8)
{
    return (int)hipMemcpyFromSymbol(host8, HIP_SYMBOL(g_hme_loop_phase), sizeof(g_hme_loop_phase));
}
#endif

}  // namespace svthip
