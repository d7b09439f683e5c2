// svt-av1-1_amd/csrc/svthip_internal.h -- what every kernel family and the C-ABI glue have in common.  The families' launch functions are
// declared per family: me_launch.h, pa_launch.h, tq_launch.h, ip_launch.h, lf_launch.h, lr_launch.h, cf_launch.h, fg_launch.h, md_launch.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/svtav1_hip.h"

#define SVTHIP_LOCAL __attribute__((visibility("hidden")))  // the library's exported symbol list stays as it is

namespace svthip {

// XCD-aware block -> work-item map for the per-superblock kernels.  The dispatcher deals consecutive workgroups round-robin over the 8
// XCDs (MI355X_MICROARCH.md: blocks b and b + 8 share an XCD), and every XCD has its own 4 MB L2: with item = blockIdx, raster
// neighbours -- whose search windows overlap by half -- land on 8 different L2s and each fetches the overlap for itself.  With
//     item = (b % 8) * ceil(n / 8) + b / 8          (grid = 8 * ceil(n / 8) blocks, items >= n exit at once)
// an XCD works through one contiguous eighth of the superblock list, so the overlapping window rows are L2 hits.  Placement is used
// for speed only: any block -> XCD assignment gives the same results.
__host__ __device__ inline uint32_t xcd_grid(uint32_t n) { return 8u * ((n + 7u) >> 3); }
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t xcd_item(uint32_t b, uint32_t n) { return (b & 7u) * ((n + 7u) >> 3) + (b >> 3); }
#endif

// Every kernel of the list gets its dynamic LDS limit raised to what the largest legal launch needs: 160 KB minus the kernel's static
// LDS.  A file that owns kernels whose dynamic LDS can pass 64 KB exports one <name>_raise_dynamic_lds() that calls this on its own
// list; svthip_create runs them once per device.  All kernels are tried; the last failure is the result.
inline hipError_t raise_dynamic_lds(const void* const* kernels, size_t n)
{
    hipError_t st = hipSuccess;
    for (size_t i = 0; i < n; i++) {
        hipFuncAttributes fa;
        hipError_t e = hipFuncGetAttributes(&fa, kernels[i]);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - (int)fa.sharedSizeBytes);
        if (e != hipSuccess) st = e;
    }
    return st;
}
template <size_t N>
hipError_t raise_dynamic_lds(const void* const (&kernels)[N]) { return raise_dynamic_lds(kernels, N); }

}  // namespace svthip
