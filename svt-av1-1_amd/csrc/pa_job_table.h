// svt-av1-1_amd/csrc/pa_job_table.h -- the job table of one launch of the kernels that work on a batch of pool pictures (me_hme.hip,
// me_ois.hip, pa_planes.hip) and how their launch functions cut a batch into launches.  Kernel side only: the C-ABI glue hands the
// launch functions its host picture arrays.
#pragma once
#include <string.h>

#include "svthip_internal.h"

namespace svthip {

// job table of one picture-analysis launch, passed by value in the kernel arguments
struct PaJobTable {
    svthip_pa_picture pic[SVTHIP_HME_MAX_JOBS];
};

inline PaJobTable pa_job_table(const svthip_pa_picture* pics, uint32_t nj)
{
    PaJobTable jt;
    memset(&jt, 0, sizeof(jt));
    for (uint32_t j = 0; j < nj; j++) jt.pic[j] = pics[j];
    return jt;
}

// pictures j0 .. of n that share one launch: the kernels take their job tables by value, SVTHIP_HME_MAX_JOBS entries each
inline uint32_t jobs_in_chunk(uint32_t n, uint32_t j0) { return n - j0 < SVTHIP_HME_MAX_JOBS ? n - j0 : SVTHIP_HME_MAX_JOBS; }

}  // namespace svthip
