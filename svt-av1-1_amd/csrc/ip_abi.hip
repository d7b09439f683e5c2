// svt-av1-1_amd/csrc/ip_abi.hip -- C-ABI glue of inter, warped, intra and chroma-from-luma prediction: the exported entries that launch
// through ip_launch.h, with their validators and shared bodies.  Host code only.
#include "svthip_glue.h"
#include "ip_launch.h"

namespace {

int32_t inter_pred_entry(svthip_ctx* ctx, const svthip_inter_planes* ref0, const svthip_inter_planes* ref1, const svthip_inter_planes* dst,
                         const svthip_inter_pu_desc* d_desc, uint32_t n_pu, uint32_t bwidth, uint32_t bheight, int bd, void* stream)
{
    TRY(check_av1_block(bwidth, bheight));
    if (n_pu == 0) return SVTHIP_OK;
    TRY(pred_check_args({ref0, ref1, dst}, d_desc));
    hipStream_t s;
    uint32_t* d_refused;
    TRY(pred_begin(ctx, {ref0, ref1, dst}, bd, n_pu, 0x0fffffffu, svthip::inter_pred_scratch_bytes, stream, &s, &d_refused));
    HIP_TRY(svthip::launch_inter_pred(*ref0, *ref1, *dst, d_desc, n_pu, (int)bwidth, (int)bheight, bd, !ctx->opt[SVTHIP_OPT_CONVOLVE_VALU],
                                      ctx->scratch[SLOT_INTER_JOBS], d_refused, s));
    return SVTHIP_OK;
}

int32_t warped_pred_entry(svthip_ctx* ctx, const svthip_inter_planes* ref, const svthip_inter_planes* dst, uint32_t pic_width, uint32_t pic_height,
                          const svthip_warp_pu_desc* d_desc, uint32_t n_pu, uint32_t bwidth, uint32_t bheight, int bd, void* stream)
{
    if (!svthip::warp_size_valid((int)bwidth, (int)bheight))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "not an AV1 block size of at least 8x8 (width %d)", (int)bwidth);
    if (n_pu == 0) return SVTHIP_OK;
    TRY(pred_check_args({ref, dst}, d_desc));
    if (!pic_width || !pic_height || pic_width > 65535u || pic_height > 65535u)
        return fail(SVTHIP_ERR_BAD_PARAMETER, "pic_width and pic_height must be 1..65535 (width %d)", (int)pic_width);
    hipStream_t s;
    uint32_t* d_refused;
    TRY(pred_begin(ctx, {ref, dst}, bd, n_pu, 0x00ffffffu, svthip::warp_scratch_bytes, stream, &s, &d_refused));
    HIP_TRY(svthip::launch_warped_pred(*ref, *dst, (int)pic_width, (int)pic_height, d_desc, n_pu, (int)bwidth, (int)bheight, bd,
                                       ctx->scratch[SLOT_INTER_JOBS], d_refused, s));
    return SVTHIP_OK;
}

// Intra prediction of transform blocks shares only the refusal counter with the two families above: it has no job list.
int32_t intra_pred_entry(svthip_ctx* ctx, const void* d_edge, void* d_dst, const svthip_intra_desc* d_desc, uint32_t n_blocks, uint32_t tx_size,
                         int bd, const uint8_t* d_src, uint32_t* d_sad, void* stream)
{
    if (!svthip::intra_tx_size_valid(tx_size)) return fail(SVTHIP_ERR_BAD_PARAMETER, "tx_size must be 0..18 (got %d)", (int)tx_size);
    if (n_blocks == 0) return SVTHIP_OK;
    TRY(check_non_null({d_edge, d_dst, d_desc}));
    TRY(check_desc_aligned(d_desc));
    if (bd > 8 && !aligned({d_edge, d_dst}, 2)) return fail(SVTHIP_ERR_BAD_PARAMETER, "16-bit planes must be 2-byte aligned");
    if (d_sad && !d_src) return fail(SVTHIP_ERR_BAD_PARAMETER, "d_sad needs d_src");
    if (d_sad && !aligned(d_sad, 4)) return fail(SVTHIP_ERR_BAD_PARAMETER, "d_sad must be 4-byte aligned");
    hipStream_t s;
    uint32_t* d_refused;
    TRY(refused_counter(ctx, stream, &s, &d_refused));
    HIP_TRY(svthip::launch_intra_pred(d_edge, d_dst, d_desc, n_blocks, (int)tx_size, bd, d_src, d_sad, d_refused, s));
    return SVTHIP_OK;
}

// Chroma-from-luma: the two predict entries and the candidates entry share the checks; only the predict entries can refuse on the device.
int32_t check_cfl_args(std::initializer_list<const void*> planes, const svthip_cfl_desc* d_desc, int bd)
{
    TRY(check_non_null(planes));
    TRY(check_non_null({d_desc}));
    TRY(check_desc_aligned(d_desc));
    if (bd > 8 && !aligned(planes, 2)) return fail(SVTHIP_ERR_BAD_PARAMETER, "16-bit planes must be 2-byte aligned");
    return SVTHIP_OK;
}

int32_t check_cfl_luma_size(uint32_t luma_w, uint32_t luma_h)
{
    return svthip::cfl_luma_size_valid(luma_w, luma_h)
               ? SVTHIP_OK
               : fail(SVTHIP_ERR_BAD_PARAMETER, "not a CfL luma size: sides 8, 16 or 32 with a ratio of at most 4 (got %dx%d)", (int)luma_w, (int)luma_h);
}

int32_t cfl_pred_entry(svthip_ctx* ctx, const void* d_luma, const void* d_cb, const void* d_cr, void* d_cb_dst, void* d_cr_dst,
                       const svthip_cfl_desc* d_desc, uint32_t n_blocks, uint32_t luma_w, uint32_t luma_h, int bd, void* stream)
{
    TRY(check_cfl_luma_size(luma_w, luma_h));
    if (n_blocks == 0) return SVTHIP_OK;
    TRY(check_cfl_args({d_luma, d_cb, d_cr, d_cb_dst, d_cr_dst}, d_desc, bd));
    hipStream_t s;
    uint32_t* d_refused;
    TRY(refused_counter(ctx, stream, &s, &d_refused));
    HIP_TRY(svthip::launch_cfl_pred(d_luma, d_cb, d_cr, d_cb_dst, d_cr_dst, d_desc, n_blocks, (int)luma_w, (int)luma_h, bd,
                                    d_refused, s));
    return SVTHIP_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- prediction

int32_t svthip_av1_convolve_sr_batch_dev(svthip_ctx* ctx, const uint8_t* d_src, uint32_t src_stride, uint8_t* d_dst, uint32_t dst_stride,
                                         const svthip_convolve_desc* d_desc, uint32_t n_blocks, uint32_t width, uint32_t height, void* stream)
{
    TRY(enter(ctx));
    TRY(check_av1_block(width, height));
    if (n_blocks == 0) return SVTHIP_OK;
    TRY(check_non_null({d_src, d_dst, d_desc}));
    TRY(check_desc_aligned(d_desc));
    hipStream_t s = call_stream(ctx, stream);
    const svthip::ConvolveLaunch L = {d_src, src_stride, nullptr, 0, d_dst, dst_stride, d_desc, n_blocks, (int)width, (int)height, 8, false, false};
    // sides that are multiples of 32: both passes as exact i8 matrix products on the matrix cores (ip_convolve_mfma.hip)
    const bool mfma = svthip::convolve_mfma_size_valid((int)width, (int)height) && !ctx->opt[SVTHIP_OPT_CONVOLVE_VALU];
    HIP_TRY(mfma ? svthip::launch_convolve_mfma(L, s) : svthip::launch_convolve_valu(L, s));
    return SVTHIP_OK;
}

int32_t svthip_av1_convolve_compound_batch_dev(svthip_ctx* ctx, const uint8_t* d_src0, uint32_t src0_stride, const uint8_t* d_src1, uint32_t src1_stride,
                                               uint8_t* d_dst, uint32_t dst_stride, const svthip_convolve_compound_desc* d_desc, uint32_t n_blocks,
                                               uint32_t width, uint32_t height, void* stream)
{
    TRY(enter(ctx));
    TRY(check_av1_block(width, height));
    if (n_blocks == 0) return SVTHIP_OK;
    TRY(check_non_null({d_src0, d_src1, d_dst, d_desc}));
    TRY(check_desc_aligned(d_desc));
    hipStream_t s = call_stream(ctx, stream);
    const svthip::ConvolveLaunch L = {d_src0, src0_stride, d_src1, src1_stride, d_dst, dst_stride, d_desc, n_blocks, (int)width, (int)height, 8, true, false};
    const bool mfma = svthip::convolve_mfma_size_valid((int)width, (int)height) && !ctx->opt[SVTHIP_OPT_CONVOLVE_VALU];
    HIP_TRY(mfma ? svthip::launch_convolve_mfma(L, s) : svthip::launch_convolve_valu(L, s));
    return SVTHIP_OK;
}

int32_t svthip_av1_highbd_convolve_batch_dev(svthip_ctx* ctx, const uint16_t* d_src0, uint32_t src0_stride, const uint16_t* d_src1, uint32_t src1_stride,
                                             uint16_t* d_dst, uint32_t dst_stride, const void* d_desc, int32_t compound, uint32_t n_blocks, uint32_t width,
                                             uint32_t height, uint32_t bit_depth, void* stream)
{
    TRY(enter(ctx));
    TRY(check_av1_block(width, height));
    TRY(check_bit_depth_10(bit_depth));
    if (n_blocks == 0) return SVTHIP_OK;
    if (!d_src0 || (compound && !d_src1) || !d_dst || !d_desc) return fail(SVTHIP_ERR_BAD_PARAMETER, "null pointer argument");
    if (!aligned(d_desc, 16) || !aligned({d_src0, d_src1, d_dst}, 2))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "descriptor array must be 16-byte aligned, planes 2-byte aligned");
    const svthip::ConvolveLaunch L = {d_src0, src0_stride, d_src1, src1_stride, d_dst, dst_stride, d_desc, n_blocks, (int)width, (int)height,
                                      (int)bit_depth, compound != 0, false};
    HIP_TRY(svthip::launch_convolve_valu(L, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t svthip_av1_inter_pred_batch_dev(svthip_ctx* ctx, const svthip_inter_planes* ref0, const svthip_inter_planes* ref1, const svthip_inter_planes* dst,
                                        const svthip_inter_pu_desc* d_desc, uint32_t n_pu, uint32_t bwidth, uint32_t bheight, void* stream)
{
    TRY(enter(ctx));
    return inter_pred_entry(ctx, ref0, ref1, dst, d_desc, n_pu, bwidth, bheight, 8, stream);
}

int32_t svthip_av1_highbd_inter_pred_batch_dev(svthip_ctx* ctx, const svthip_inter_planes* ref0, const svthip_inter_planes* ref1,
                                               const svthip_inter_planes* dst, const svthip_inter_pu_desc* d_desc, uint32_t n_pu, uint32_t bwidth,
                                               uint32_t bheight, uint32_t bit_depth, void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return inter_pred_entry(ctx, ref0, ref1, dst, d_desc, n_pu, bwidth, bheight, (int)bit_depth, stream);
}

int32_t svthip_av1_warped_pred_batch_dev(svthip_ctx* ctx, const svthip_inter_planes* ref, const svthip_inter_planes* dst, uint32_t pic_width,
                                         uint32_t pic_height, const svthip_warp_pu_desc* d_desc, uint32_t n_pu, uint32_t bwidth, uint32_t bheight,
                                         void* stream)
{
    TRY(enter(ctx));
    return warped_pred_entry(ctx, ref, dst, pic_width, pic_height, d_desc, n_pu, bwidth, bheight, 8, stream);
}

int32_t svthip_av1_highbd_warped_pred_batch_dev(svthip_ctx* ctx, const svthip_inter_planes* ref, const svthip_inter_planes* dst, uint32_t pic_width,
                                                uint32_t pic_height, const svthip_warp_pu_desc* d_desc, uint32_t n_pu, uint32_t bwidth,
                                                uint32_t bheight, uint32_t bit_depth, void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return warped_pred_entry(ctx, ref, dst, pic_width, pic_height, d_desc, n_pu, bwidth, bheight, (int)bit_depth, stream);
}

int32_t svthip_av1_intra_pred_batch_dev(svthip_ctx* ctx, const uint8_t* d_edge, uint8_t* d_dst, const svthip_intra_desc* d_desc, uint32_t n_blocks,
                                        uint32_t tx_size, const uint8_t* d_src, uint32_t* d_sad, void* stream)
{
    TRY(enter(ctx));
    return intra_pred_entry(ctx, d_edge, d_dst, d_desc, n_blocks, tx_size, 8, d_src, d_sad, stream);
}

int32_t svthip_av1_highbd_intra_pred_batch_dev(svthip_ctx* ctx, const uint16_t* d_edge, uint16_t* d_dst, const svthip_intra_desc* d_desc,
                                               uint32_t n_blocks, uint32_t tx_size, uint32_t bit_depth, void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return intra_pred_entry(ctx, d_edge, d_dst, d_desc, n_blocks, tx_size, (int)bit_depth, nullptr, nullptr, stream);
}

int32_t svthip_av1_cfl_pred_batch_dev(svthip_ctx* ctx, const uint8_t* d_luma, const uint8_t* d_cb, const uint8_t* d_cr, uint8_t* d_cb_dst,
                                      uint8_t* d_cr_dst, const svthip_cfl_desc* d_desc, uint32_t n_blocks, uint32_t luma_w, uint32_t luma_h,
                                      void* stream)
{
    TRY(enter(ctx));
    return cfl_pred_entry(ctx, d_luma, d_cb, d_cr, d_cb_dst, d_cr_dst, d_desc, n_blocks, luma_w, luma_h, 8, stream);
}

int32_t svthip_av1_highbd_cfl_pred_batch_dev(svthip_ctx* ctx, const uint16_t* d_luma, const uint16_t* d_cb, const uint16_t* d_cr,
                                             uint16_t* d_cb_dst, uint16_t* d_cr_dst, const svthip_cfl_desc* d_desc, uint32_t n_blocks,
                                             uint32_t luma_w, uint32_t luma_h, uint32_t bit_depth, void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return cfl_pred_entry(ctx, d_luma, d_cb, d_cr, d_cb_dst, d_cr_dst, d_desc, n_blocks, luma_w, luma_h, (int)bit_depth, stream);
}

int32_t svthip_av1_cfl_alpha_candidates_batch_dev(svthip_ctx* ctx, const uint8_t* d_luma, const uint8_t* d_cb_dc, const uint8_t* d_cr_dc,
                                                  const svthip_cfl_desc* d_desc, uint32_t n_blocks, uint32_t luma_w, uint32_t luma_h,
                                                  uint8_t* d_candidates, void* stream)
{
    TRY(enter(ctx));
    TRY(check_cfl_luma_size(luma_w, luma_h));
    if (n_blocks == 0) return SVTHIP_OK;
    TRY(check_cfl_args({d_luma, d_cb_dc, d_cr_dc, d_candidates}, d_desc, 8));
    HIP_TRY(svthip::launch_cfl_candidates(d_luma, d_cb_dc, d_cr_dc, d_desc, n_blocks, (int)luma_w, (int)luma_h, d_candidates, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t svthip_cfl_alpha_decision_batch_dev(svthip_ctx* ctx, const uint64_t* d_distortion, const uint32_t* d_bits, uint32_t dist_shift,
                                            const int32_t* d_alpha_bits, const svthip_cfl_decision_job* d_job, uint32_t n_blocks,
                                            svthip_cfl_decision* d_out, void* stream)
{
    TRY(enter(ctx));
    if (dist_shift > 63) return fail(SVTHIP_ERR_BAD_PARAMETER, "dist_shift must be 0..63 (got %u)", (unsigned)dist_shift);
    if (n_blocks == 0) return SVTHIP_OK;
    TRY(check_non_null({d_distortion, d_bits, d_alpha_bits, d_job, d_out}));
    if (!aligned({d_job, d_out}, 16)) return fail(SVTHIP_ERR_BAD_PARAMETER, "job and decision arrays must be 16-byte aligned");
    if (!aligned(d_distortion, 8) || !aligned({d_bits, d_alpha_bits}, 4))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "d_distortion must be 8-byte, d_bits and d_alpha_bits 4-byte aligned");
    HIP_TRY(svthip::launch_cfl_decision(d_distortion, d_bits, dist_shift, d_alpha_bits, d_job, n_blocks, d_out, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

}  // extern "C"
