// svt-av1-1_amd/csrc/md_part.hip
//
// Mode decision's partition decision on the device, gfx950: the launches of md_part_kernels.h.  Replaces what mode_decision_sb
// (Source/Lib/Codec/EbProductCodingLoop.c:2823-2873) does with the block costs of a superblock -- d1_non_square_block_decision and
// d2_inter_depth_block_decision (Codec/EbFullLoop.c:2086-2108, :2368-2437) -- for all superblocks of a picture in one launch, lists the
// final blocks as EncodePass walks them (Codec/EbCodingLoop.c:3051-3069, :4111-4114), and copies their winner tiles into one picture in a
// second.  The geometry is computed from the block index on both sides; svthip_md_partition_geometry is the same function on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svtav1_hip.h"
#include "md_launch.h"
#include "md_part_kernels.h"

namespace svthip {

uint32_t md_part_geometry(uint32_t sb_size, svthip_md_partition_block* out, uint32_t max)
{
    if (sb_size != 64u && sb_size != 128u) return 0;
    const uint32_t n = md_part_blocks(sb_size);
    for (uint32_t i = 0; out && i < n && i < max; i++) out[i] = md_part_geom(sb_size, i);
    return n;
}

hipError_t launch_md_part_decide(const MdPartCall& C, hipStream_t s)
{
    MdPartArgs A;
    A.sb = C.sb, A.leaf = C.leaf, A.decision = C.decision;
    A.n_sb = C.n_sb, A.n_leaf = C.n_leaf, A.n_decision = C.n_decision, A.intra = C.slice_is_intra ? 1u : 0u;
    const int rows[4] = {0, 4, 8, 10};   // below 8x8, PARTITION_TYPES, EXT_PARTITION_TYPES - 2, EXT_PARTITION_TYPES
    for (int r = 0; r < 4; r++) A.bits[r][0] = C.partition_fac_bits[rows[r] * 11 + 0], A.bits[r][1] = C.partition_fac_bits[rows[r] * 11 + 3];
    A.result = C.result, A.final_ = C.final_, A.final_count = C.final_count, A.refused = C.refused;
    if (C.sb_size == 128u) hipLaunchKernelGGL(md_part_decide_kernel<128>, dim3(C.n_sb), dim3(MD_PART_THREADS), 0, s, A);
    else hipLaunchKernelGGL(md_part_decide_kernel<64>, dim3(C.n_sb), dim3(MD_PART_THREADS), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_md_part_compose(const MdPartCall& C, hipStream_t s)
{
    MdPartComposeArgs A;
    A.leaf = C.leaf, A.final_ = C.final_, A.final_count = C.final_count, A.n_sb = C.n_sb, A.n_leaf = C.n_leaf, A.max_final = md_part_max_final(C.sb_size);
    void* const pool[3] = {C.pool.y, C.pool.cb, C.pool.cr};
    void* const dst[3] = {C.dst.y, C.dst.cb, C.dst.cr};
    for (int p = 0; p < 3; p++) A.pool[p] = static_cast<const uint8_t*>(pool[p]), A.dst[p] = static_cast<uint8_t*>(dst[p]);
    A.pool_stride[0] = C.pool.y_stride, A.pool_stride[1] = C.pool.c_stride, A.dst_stride[0] = C.dst.y_stride, A.dst_stride[1] = C.dst.c_stride;
    A.pool_w = C.pool_width, A.pool_h = C.pool_height, A.w = C.width, A.h = C.height;
    A.refused = C.refused;
    hipLaunchKernelGGL(md_part_compose_kernel, dim3(C.n_sb, md_part_compose_slices(C.n_sb)), dim3(MD_PART_THREADS), 0, s, A);
    return hipGetLastError();
}

}  // namespace svthip
