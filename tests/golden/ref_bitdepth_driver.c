/*
 * tests/golden/ref_bitdepth_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own UnPack2D, extract_8bit_data, Pack2D_SRC and CompressedPackLcu (Codec/EbPictureOperators.c:550-720), its
 * PsnrCalculations (Codec/EbEncDecProcess.c:775-1133) and its AV1InterPrediction10BitMD (Codec/EbInterPrediction.c:1477-) for
 * tests/golden/make_golden_bitdepth.py and tests/test_bitdepth_vs_ref.py.  Contains no reference code: it builds the objects those functions
 * read and calls them the way their callers do.
 *   drv_unpack / drv_extract8      the three planes of a picture, one call per plane as Codec/EbEncHandle.c:2954-2985
 *   drv_pack / drv_pack_compressed SB by SB (64 x 64 clipped to the picture) into an SB-sized 16-bit buffer as Codec/EbCodingLoop.c:2888-2974
 *                                  does, with the same buffer offsets -- the compressed plane addressed as :2901, :2912, :2923 -- and, as
 *                                  there, strideCr with the Cb plane; the SB buffer is then copied into the caller's 16-bit planes
 *   drv_psnr                       PsnrCalculations on zeroed control sets that carry what it reads: encoder_bit_depth, ten_bit_format, the
 *                                  luma / chroma dimensions, is_used_as_reference_flag = 0, recon_picture_ptr / recon_picture16bit_ptr and
 *                                  enhanced_picture_ptr.  mode 0: 8 bits; 1: 16 bits against 8-bit + unpacked 2-bit planes; 2: against 8-bit +
 *                                  compressed planes.  out = luma_sse, cb_sse, cr_sse as the function leaves them
 *   drv_md_predict                 AV1InterPrediction10BitMD of one PU from two padded 16-bit references into 8-bit prediction planes, with
 *                                  the two local 8-bit block buffers of the motion-compensation context; the state around it as
 *                                  tests/golden/ref_inter_pred_driver.c builds it for av1_inter_prediction
 * asm_type is ASM_NON_AVX2 everywhere.  What that selects (Codec/EbPackUnPack.h): for planes whose width is a multiple of 4 and whose height
 * is even -- all of them here -- UnPack2D, extract_8bit_data and Pack2D_SRC are the SSE2 intrinsic forms for either asm_type;
 * CompressedPackLcu is the C CompressedPackmsb; the block copy inside AV1InterPrediction10BitMD is the SSE2 one for either asm_type.  The
 * fixture's samples with bits above bit 9 show that the intrinsic forms do what the casts of the C text do.
 */
#define RTCD_C
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "EbDefinitions.h"
#include "aom_dsp_rtcd.h"
#include "EbCodingUnit.h"
#include "EbInterPrediction.h"
#include "EbMcp.h"
#include "EbModeDecisionProcess.h"
#include "EbPictureBufferDesc.h"
#include "EbPictureControlSet.h"
#include "EbPictureOperators.h"
#include "EbSequenceControlSet.h"
#include "EbUtility.h"

void PsnrCalculations(PictureControlSet_t *picture_control_set_ptr, SequenceControlSet_t *sequence_control_set_ptr);
EbErrorType AV1InterPrediction10BitMD(uint32_t interp_filters, PictureControlSet_t *picture_control_set_ptr, uint8_t ref_frame_type,
                                      ModeDecisionContext_t *md_context_ptr, CodingUnit_t *cu_ptr, MvUnit_t *mv_unit, uint16_t pu_origin_x,
                                      uint16_t pu_origin_y, uint8_t bwidth, uint8_t bheight, EbPictureBufferDesc_t *ref_pic_list0,
                                      EbPictureBufferDesc_t *ref_pic_list1, EbPictureBufferDesc_t *prediction_ptr, uint16_t dst_origin_x,
                                      uint16_t dst_origin_y, EbAsm asm_type);
void asmSetConvolveAsmTable(void);
void av1_set_ref_frame(MvReferenceFrame *rf, int8_t ref_frame_type);
extern BlockGeom blk_geom_mds[];

int drv_init(void)
{
    av1_convolve_2d_sr = av1_convolve_2d_sr_c;
    av1_convolve_x_sr = av1_convolve_x_sr_c;
    av1_convolve_y_sr = av1_convolve_y_sr_c;
    av1_convolve_2d_copy_sr = av1_convolve_2d_copy_sr_c;
    av1_jnt_convolve_2d = av1_jnt_convolve_2d_c;
    av1_jnt_convolve_x = av1_jnt_convolve_x_c;
    av1_jnt_convolve_y = av1_jnt_convolve_y_c;
    av1_jnt_convolve_2d_copy = av1_jnt_convolve_2d_copy_c;
    asmSetConvolveAsmTable();
    return 0;
}

/* planes: tight (stride = width) arrays of the picture's three planes */
void drv_unpack(int w, int h, uint16_t *const in16[3], uint8_t *const out8[3], uint8_t *const outn[3])
{
    for (int p = 0; p < 3; p++) {
        const int pw = p ? w / 2 : w, ph = p ? h / 2 : h;
        UnPack2D(in16[p], pw, out8[p], pw, outn[p], pw, pw, ph, ASM_NON_AVX2);
    }
}

void drv_extract8(int w, int h, uint16_t *const in16[3], uint8_t *const out8[3])
{
    for (int p = 0; p < 3; p++) {
        const int pw = p ? w / 2 : w, ph = p ? h / 2 : h;
        extract_8bit_data(in16[p], pw, out8[p], pw, pw, ph, ASM_NON_AVX2);
    }
}

static void copy_sb(uint16_t *dst, int dst_stride, const uint16_t *sb, int sb_stride, int sb_w, int sb_h)
{
    for (int y = 0; y < sb_h; y++) memcpy(dst + (size_t)y * dst_stride, sb + (size_t)y * sb_stride, sizeof(uint16_t) * sb_w);
}

/* compressed == 0: inn are unpacked 2-bit planes (stride = width); else the compressed planes */
void drv_pack(int compressed, int w, int h, uint8_t *const in8[3], uint8_t *const inn[3], uint16_t *const out16[3])
{
    static uint16_t sb_y[64 * 64], sb_cb[32 * 32], sb_cr[32 * 32];
    const int strideY = w, strideCb = w / 2, strideCr = w / 2, strideBitIncY = w, strideBitIncCb = w / 2, strideBitIncCr = w / 2;
    for (int sb_origin_y = 0; sb_origin_y < h; sb_origin_y += 64)
        for (int sb_origin_x = 0; sb_origin_x < w; sb_origin_x += 64) {
            const int sb_width = w - sb_origin_x < 64 ? w - sb_origin_x : 64, sb_height = h - sb_origin_y < 64 ? h - sb_origin_y : 64;
            const uint32_t inputLumaOffset = sb_origin_y * strideY + sb_origin_x;
            const uint32_t inputCbOffset = (sb_origin_y >> 1) * strideCb + (sb_origin_x >> 1);
            const uint32_t inputCrOffset = (sb_origin_y >> 1) * strideCr + (sb_origin_x >> 1);
            if (compressed) {
                const uint16_t luma2BitWidth = w / 4, chroma2BitWidth = w / 8;
                CompressedPackLcu(in8[0] + inputLumaOffset, strideY, inn[0] + sb_origin_y * luma2BitWidth + (sb_origin_x / 4) * sb_height, sb_width / 4, sb_y,
                                  64, sb_width, sb_height, ASM_NON_AVX2);
                CompressedPackLcu(in8[1] + inputCbOffset, strideCb, inn[1] + sb_origin_y / 2 * chroma2BitWidth + (sb_origin_x / 8) * (sb_height / 2),
                                  sb_width / 8, sb_cb, 32, sb_width >> 1, sb_height >> 1, ASM_NON_AVX2);
                CompressedPackLcu(in8[2] + inputCrOffset, strideCr, inn[2] + sb_origin_y / 2 * chroma2BitWidth + (sb_origin_x / 8) * (sb_height / 2),
                                  sb_width / 8, sb_cr, 32, sb_width >> 1, sb_height >> 1, ASM_NON_AVX2);
            } else {
                const uint32_t inputBitIncLumaOffset = sb_origin_y * strideBitIncY + sb_origin_x;
                const uint32_t inputBitIncCbOffset = (sb_origin_y >> 1) * strideBitIncCb + (sb_origin_x >> 1);
                const uint32_t inputBitIncCrOffset = (sb_origin_y >> 1) * strideBitIncCr + (sb_origin_x >> 1);
                Pack2D_SRC(in8[0] + inputLumaOffset, strideY, inn[0] + inputBitIncLumaOffset, strideBitIncY, sb_y, 64, sb_width, sb_height, ASM_NON_AVX2);
                Pack2D_SRC(in8[1] + inputCbOffset, strideCr, inn[1] + inputBitIncCbOffset, strideBitIncCr, sb_cb, 32, sb_width >> 1, sb_height >> 1,
                           ASM_NON_AVX2);
                Pack2D_SRC(in8[2] + inputCrOffset, strideCr, inn[2] + inputBitIncCrOffset, strideBitIncCr, sb_cr, 32, sb_width >> 1, sb_height >> 1,
                           ASM_NON_AVX2);
            }
            copy_sb(out16[0] + inputLumaOffset, w, sb_y, 64, sb_width, sb_height);
            copy_sb(out16[1] + inputCbOffset, w / 2, sb_cb, 32, sb_width >> 1, sb_height >> 1);
            copy_sb(out16[2] + inputCrOffset, w / 2, sb_cr, 32, sb_width >> 1, sb_height >> 1);
        }
}

static void tight_desc(EbPictureBufferDesc_t *d, int w, void *const planes[3], uint8_t *const planes_n[3])
{
    memset(d, 0, sizeof(*d));
    d->bufferY = (EbByte)planes[0], d->bufferCb = (EbByte)planes[1], d->bufferCr = (EbByte)planes[2];
    d->strideY = (uint16_t)w, d->strideCb = d->strideCr = (uint16_t)(w / 2);
    if (planes_n) {
        d->bufferBitIncY = planes_n[0], d->bufferBitIncCb = planes_n[1], d->bufferBitIncCr = planes_n[2];
        d->strideBitIncY = (uint16_t)w, d->strideBitIncCb = d->strideBitIncCr = (uint16_t)(w / 2);
    }
}

void drv_psnr(int mode, int w, int h, void *const recon[3], uint8_t *const src8[3], uint8_t *const srcn[3], uint32_t out[3])
{
    static SequenceControlSet_t scs;
    static PictureParentControlSet_t ppcs;
    static PictureControlSet_t pcs;
    EbPictureBufferDesc_t recon_desc, input_desc;
    memset(&scs, 0, sizeof(scs));
    memset(&ppcs, 0, sizeof(ppcs));
    memset(&pcs, 0, sizeof(pcs));
    scs.static_config.encoder_bit_depth = mode ? EB_10BIT : EB_8BIT;
    scs.static_config.ten_bit_format = mode == 2;
    scs.luma_width = (uint16_t)w, scs.luma_height = (uint16_t)h, scs.chroma_width = (uint16_t)(w / 2), scs.chroma_height = (uint16_t)(h / 2);
    tight_desc(&recon_desc, w, recon, NULL);
    tight_desc(&input_desc, w, (void *const *)src8, mode ? srcn : NULL);
    ppcs.is_used_as_reference_flag = EB_FALSE;
    ppcs.enhanced_picture_ptr = &input_desc;
    pcs.parent_pcs_ptr = &ppcs;
    pcs.recon_picture_ptr = pcs.recon_picture16bit_ptr = &recon_desc;
    PsnrCalculations(&pcs, &scs);
    out[0] = ppcs.luma_sse, out[1] = ppcs.cb_sse, out[2] = ppcs.cr_sse;
}

static void set_buf(EbPictureBufferDesc_t *b, void *const planes[3], const int32_t strides[2], int border)
{
    memset(b, 0, sizeof(*b));
    b->bufferY = (EbByte)planes[0];
    b->bufferCb = (EbByte)planes[1];
    b->bufferCr = (EbByte)planes[2];
    b->strideY = (uint16_t)strides[0];
    b->strideCb = b->strideCr = (uint16_t)strides[1];
    b->origin_x = b->origin_y = (uint16_t)border;
}

/* pu[], nb[], planes, strides, border, pborder as drv_predict of ref_inter_pred_driver.c; the references are 16-bit, the prediction 8-bit.
 * local_fill: the byte the two local block buffers hold before the call (what an earlier call left there in the encoder) */
int drv_md_predict(const int32_t *pu, const int32_t *nb, int pic_w, int pic_h, void *const *planes, const int32_t *strides, int border, int pborder,
                   int local_fill)
{
    static SequenceControlSet_t scs;
    static PictureParentControlSet_t ppcs;
    static PictureControlSet_t pcs;
    static CodingUnit_t cu;
    static MacroBlockD xd;
    static ModeDecisionContext_t md;
    static InterPredictionContext_t ipc;
    static MotionCompensationPredictionContext_t mcp;
    static uint8_t local[2][3][(128 + 16) * (128 + 16)];
    EbPictureBufferDesc_t local_desc[2];
    memset(&scs, 0, sizeof(scs));
    memset(&ppcs, 0, sizeof(ppcs));
    memset(&pcs, 0, sizeof(pcs));
    memset(&cu, 0, sizeof(cu));
    memset(&xd, 0, sizeof(xd));
    memset(&md, 0, sizeof(md));
    memset(&ipc, 0, sizeof(ipc));
    memset(&mcp, 0, sizeof(mcp));
    memset(local, local_fill, sizeof(local));
    for (int l = 0; l < 2; l++) {
        memset(&local_desc[l], 0, sizeof(local_desc[l]));
        local_desc[l].bufferY = local[l][0], local_desc[l].bufferCb = local[l][1], local_desc[l].bufferCr = local[l][2];
        local_desc[l].strideY = 128 + 16, local_desc[l].strideCb = local_desc[l].strideCr = 64 + 16;
    }
    mcp.local_reference_block8_bitl0 = &local_desc[0];
    mcp.local_reference_block8_bitl1 = &local_desc[1];
    ipc.mcp_context = &mcp;
    md.inter_prediction_context = &ipc;
    scs.picture_width_in_sb = (uint16_t)((pic_w + 63) / 64);
    ppcs.sequence_control_set_ptr = &scs;
    pcs.parent_pcs_ptr = &ppcs;
    const int stride = scs.picture_width_in_sb * 16, rows = (pic_h + 3) / 4, margin = stride + 1;
    const size_t n_mi = (size_t)(rows + 2) * stride + 2;
    ModeInfo *mip = (ModeInfo *)calloc(n_mi, sizeof(ModeInfo));
    ModeInfo **grid = (ModeInfo **)calloc((size_t)rows * stride, sizeof(ModeInfo *));
    if (!mip || !grid) return -1;
    for (size_t i = 0; i < (size_t)rows * stride; i++) grid[i] = mip + margin + i;
    pcs.mi_grid_base = grid;
    const int mi_x = pu[0] >> 2, mi_y = pu[1] >> 2;
    for (int k = 0; k < 3; k++) {
        const int row = k < 2 ? -1 : 0, col = k == 1 ? 0 : -1;
        MbModeInfo *m = &mip[margin + (mi_y + row) * stride + mi_x + col].mbmi;
        m->ref_frame[0] = (MvReferenceFrame)nb[3 * k];
        m->mv[0].as_mv.row = (int16_t)nb[3 * k + 1];
        m->mv[0].as_mv.col = (int16_t)nb[3 * k + 2];
    }
    xd.mb_to_left_edge = pu[14];
    xd.mb_to_right_edge = pu[15];
    xd.mb_to_top_edge = pu[16];
    xd.mb_to_bottom_edge = pu[17];
    BlockGeom *g = &blk_geom_mds[0];
    memset(g, 0, sizeof(*g));
    g->bsize = (BlockSize)pu[6];
    g->bwidth = (uint8_t)pu[4];
    g->bheight = (uint8_t)pu[5];
    g->bwidth_uv = (uint8_t)(pu[4] >> 1 > 4 ? pu[4] >> 1 : 4);
    g->bheight_uv = (uint8_t)(pu[5] >> 1 > 4 ? pu[5] >> 1 : 4);
    g->has_uv = (uint8_t)pu[18];
    cu.av1xd = &xd;
    cu.mds_idx = 0;
    cu.interp_filters = (uint32_t)pu[7];
    MvUnit_t mvu;
    memset(&mvu, 0, sizeof(mvu));
    mvu.predDirection = (uint8_t)pu[9];
    mvu.mv[0].y = (int16_t)pu[10];
    mvu.mv[0].x = (int16_t)pu[11];
    mvu.mv[1].y = (int16_t)pu[12];
    mvu.mv[1].x = (int16_t)pu[13];
    EbPictureBufferDesc_t r0, r1, pr;
    set_buf(&r0, planes + 0, strides + 0, border);
    set_buf(&r1, planes + 3, strides + 2, border);
    set_buf(&pr, planes + 6, strides + 4, pborder);
    AV1InterPrediction10BitMD((uint32_t)pu[7], &pcs, (uint8_t)pu[8], &md, &cu, &mvu, (uint16_t)pu[0], (uint16_t)pu[1], (uint8_t)pu[4], (uint8_t)pu[5], &r0,
                              &r1, &pr, (uint16_t)pu[2], (uint16_t)pu[3], ASM_NON_AVX2);
    free(grid);
    free(mip);
    return 0;
}
