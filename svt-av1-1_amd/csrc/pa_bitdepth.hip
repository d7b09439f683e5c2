// svt-av1-1_amd/csrc/pa_bitdepth.hip
//
// The 10-bit picture forms of pictures that are already in device memory, gfx950: the launches of pa_bitdepth_kernels.h.  Replaces, for the
// three planes of whole 4:2:0 pictures at once, UnPack2D as the reference applies it to its input (Codec/EbEncHandle.c:2941-2986) and
// UnPack8BitData as it copies 16-bit reference blocks for 8-bit mode decision (Codec/EbInterPrediction.c:1447-1473), Pack2D_SRC and
// CompressedPackLcu as the 16-bit encode pass rebuilds its source per SB (Codec/EbCodingLoop.c:2883-2981), and PsnrCalculations
// (Codec/EbEncDecProcess.c:775-1133).  Every entry is one launch over all planes and pictures; the SSE entries add a one-wave finish
// on the same stream.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/svtav1_hip.h"
#include "pa_launch.h"
#include "pa_bitdepth_kernels.h"

namespace svthip {

namespace {

// the job table of a launch: stream k of the kernel is described by streams[k] (n entries each; nullptr: the kernel has no such stream)
PaBdTable pa_bd_table(uint32_t w, uint32_t h, uint32_t n, bool compressed, const svthip_planes* const (&streams)[3])
{
    PaBdTable t;
    memset(&t, 0, sizeof(t));
    pa_bd_geometry(&t, w, h, compressed);
    for (uint32_t j = 0; j < n; j++)
        for (int k = 0; k < 3; k++)
            for (int p = 0; p < 3 && streams[k]; p++) t.off[j][k][p] = streams[k][j].offset[p], t.stride[j][k][p] = streams[k][j].stride[p];
    return t;
}

}  // namespace

size_t pa_sse_partial_bytes(uint32_t w, uint32_t h, uint32_t n)
{
    PaBdTable t;
    return sizeof(uint64_t) * n * pa_bd_geometry(&t, w, h, false);   // the plain forms have the larger grid
}

hipError_t launch_pa_unpack_10bit(const uint16_t* in16, const svthip_planes* in16_planes, uint8_t* out8, const svthip_planes* out8_planes, uint8_t* outn,
                                  const svthip_planes* outn_planes, uint32_t w, uint32_t h, uint32_t n, hipStream_t s)
{
    const PaBdTable t = pa_bd_table(w, h, n, false, {in16_planes, out8_planes, outn ? outn_planes : nullptr});
    if (outn)
        hipLaunchKernelGGL(pa_bd_unpack_kernel<true>, dim3(n * t.block0[3]), dim3(PA_BD_LANES), 0, s, t, in16, out8, outn);
    else
        hipLaunchKernelGGL(pa_bd_unpack_kernel<false>, dim3(n * t.block0[3]), dim3(PA_BD_LANES), 0, s, t, in16, out8, outn);
    return hipGetLastError();
}

hipError_t launch_pa_pack_10bit(const uint8_t* in8, const svthip_planes* in8_planes, const uint8_t* inn, const svthip_planes* inn_planes, bool compressed,
                                uint16_t* out16, const svthip_planes* out16_planes, uint32_t w, uint32_t h, uint32_t n, hipStream_t s)
{
    const PaBdTable t = pa_bd_table(w, h, n, compressed, {in8_planes, inn_planes, out16_planes});
    if (compressed)
        hipLaunchKernelGGL(pa_bd_pack_kernel<true>, dim3(n * t.block0[3]), dim3(PA_BD_LANES), 0, s, t, in8, inn, out16);
    else
        hipLaunchKernelGGL(pa_bd_pack_kernel<false>, dim3(n * t.block0[3]), dim3(PA_BD_LANES), 0, s, t, in8, inn, out16);
    return hipGetLastError();
}

hipError_t launch_pa_picture_sse(int form, const void* recon, const svthip_planes* recon_planes, const void* src, const svthip_planes* src_planes,
                                 const uint8_t* srcn, const svthip_planes* srcn_planes, uint32_t w, uint32_t h, uint32_t n, uint64_t* partial, uint64_t* sse,
                                 hipStream_t s)
{
    const bool split = form == PA_BD_SSE_UNPACKED || form == PA_BD_SSE_COMPRESSED;
    const PaBdTable t = pa_bd_table(w, h, n, form == PA_BD_SSE_COMPRESSED, {recon_planes, src_planes, split ? srcn_planes : nullptr});
    const dim3 grid(n * t.block0[3]), block(PA_BD_LANES);
    switch (form) {
    case PA_BD_SSE_8: hipLaunchKernelGGL(pa_bd_sse_kernel<PA_BD_SSE_8>, grid, block, 0, s, t, recon, src, srcn, partial); break;
    case PA_BD_SSE_16: hipLaunchKernelGGL(pa_bd_sse_kernel<PA_BD_SSE_16>, grid, block, 0, s, t, recon, src, srcn, partial); break;
    case PA_BD_SSE_UNPACKED: hipLaunchKernelGGL(pa_bd_sse_kernel<PA_BD_SSE_UNPACKED>, grid, block, 0, s, t, recon, src, srcn, partial); break;
    default: hipLaunchKernelGGL(pa_bd_sse_kernel<PA_BD_SSE_COMPRESSED>, grid, block, 0, s, t, recon, src, srcn, partial); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pa_bd_sse_finish_kernel, dim3(3, n), dim3(64), 0, s, t, (const uint64_t*)partial, sse);
    return hipGetLastError();
}

}  // namespace svthip
