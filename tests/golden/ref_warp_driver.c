/*
 * tests/golden/ref_warp_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own warped_motion_prediction (Codec/EbInterPrediction.c:2528, 8 and 10 bits) and get_shear_params
 * (Codec/EbWarpedMotion.c:344) for tests/golden/make_golden_warp.py.  Contains no reference code: it builds the state the two functions
 * read and calls them.
 *   - block geometry: a BlockGeom filled the way md_scan_all_blks fills it (bwidth / bheight, bwidth_uv = MAX(4, bwidth >> 1), bheight_uv,
 *     has_uv); build_blk_geom itself cannot run in this build (it calls Log2f_SSE2, which exists only in the reference's NASM sources);
 *   - CodingUnit_t: av1xd with the four mb_to_*_edge values (read by the translational chroma of blocks below 16x16);
 *   - MvUnit_t: predDirection = UNI_PRED_LIST_0 and mv[REF_LIST_0];
 *   - EbWarpedMotionParams: wmtype, wmmat[0..5], alpha .. delta;
 *   - EbPictureBufferDesc_t for the reference (with width / height, which the warp clamps to) and the prediction (caller-owned planes).
 * The RTCD pointers the convolution dispatch tables copy are set to the C kernels.
 */
#define RTCD_C
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "EbDefinitions.h"
#include "aom_dsp_rtcd.h"
#include "EbCodingUnit.h"
#include "EbInterPrediction.h"
#include "EbPictureBufferDesc.h"
#include "EbUtility.h"
#include "EbWarpedMotion.h"

void asmSetConvolveAsmTable(void);
void asmSetConvolveHbdAsmTable(void);

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
    av1_highbd_convolve_2d_sr = av1_highbd_convolve_2d_sr_c;
    av1_highbd_convolve_x_sr = av1_highbd_convolve_x_sr_c;
    av1_highbd_convolve_y_sr = av1_highbd_convolve_y_sr_c;
    av1_highbd_convolve_2d_copy_sr = av1_highbd_convolve_2d_copy_sr_c;
    av1_highbd_jnt_convolve_2d = av1_highbd_jnt_convolve_2d_c;
    av1_highbd_jnt_convolve_x = av1_highbd_jnt_convolve_x_c;
    av1_highbd_jnt_convolve_y = av1_highbd_jnt_convolve_y_c;
    av1_highbd_jnt_convolve_2d_copy = av1_highbd_jnt_convolve_2d_copy_c;
    asmSetConvolveAsmTable();
    asmSetConvolveHbdAsmTable();
    return 0;
}

/* get_shear_params on wmmat[0..5]; out[0..3] = alpha, beta, gamma, delta as the function left them (0 where it returned before writing) */
int drv_shear(const int32_t *wmmat, int32_t *out)
{
    EbWarpedMotionParams wm;
    memset(&wm, 0, sizeof(wm));
    wm.wmtype = AFFINE;
    for (int i = 0; i < 6; i++) wm.wmmat[i] = wmmat[i];
    const int ok = get_shear_params(&wm);
    out[0] = wm.alpha;
    out[1] = wm.beta;
    out[2] = wm.gamma;
    out[3] = wm.delta;
    return ok;
}

static void set_buf(EbPictureBufferDesc_t *b, void *const planes[3], const int32_t strides[2], int border, int width, int height)
{
    memset(b, 0, sizeof(*b));
    b->bufferY = (EbByte)planes[0];
    b->bufferCb = (EbByte)planes[1];
    b->bufferCr = (EbByte)planes[2];
    b->strideY = (uint16_t)strides[0];
    b->strideCb = b->strideCr = (uint16_t)strides[1];
    b->origin_x = b->origin_y = (uint16_t)border;
    b->width = (uint16_t)width;
    b->height = (uint16_t)height;
}

/* One call.  pu[] = pu_x, pu_y, dst_x, dst_y, bw, bh, has_uv, mv_row, mv_col, edge_left, edge_right, edge_top, edge_bottom, wmtype,
 * wmmat[0..5], alpha, beta, gamma, delta.  planes: ref Y/Cb/Cr, pred Y/Cb/Cr; strides: luma / chroma of each; border: luma padding of the
 * reference (origin_x = origin_y), pborder: of the prediction. */
int drv_warp_predict(int bit_depth, const int32_t *pu, int pic_w, int pic_h, void *const *planes, const int32_t *strides, int border, int pborder)
{
    static CodingUnit_t cu;
    static MacroBlockD xd;
    BlockGeom g;
    memset(&cu, 0, sizeof(cu));
    memset(&xd, 0, sizeof(xd));
    memset(&g, 0, sizeof(g));
    xd.mb_to_left_edge = pu[9];
    xd.mb_to_right_edge = pu[10];
    xd.mb_to_top_edge = pu[11];
    xd.mb_to_bottom_edge = pu[12];
    cu.av1xd = &xd;
    g.bwidth = (uint8_t)pu[4];
    g.bheight = (uint8_t)pu[5];
    g.bwidth_uv = (uint8_t)(pu[4] >> 1 > 4 ? pu[4] >> 1 : 4);
    g.bheight_uv = (uint8_t)(pu[5] >> 1 > 4 ? pu[5] >> 1 : 4);
    g.has_uv = (uint8_t)pu[6];
    MvUnit_t mvu;
    memset(&mvu, 0, sizeof(mvu));
    mvu.predDirection = UNI_PRED_LIST_0;
    mvu.mv[REF_LIST_0].y = (int16_t)pu[7];
    mvu.mv[REF_LIST_0].x = (int16_t)pu[8];
    EbWarpedMotionParams wm;
    memset(&wm, 0, sizeof(wm));
    wm.wmtype = (TransformationType)pu[13];
    for (int i = 0; i < 6; i++) wm.wmmat[i] = pu[14 + i];
    wm.alpha = (int16_t)pu[20];
    wm.beta = (int16_t)pu[21];
    wm.gamma = (int16_t)pu[22];
    wm.delta = (int16_t)pu[23];
    EbPictureBufferDesc_t r0, pr;
    set_buf(&r0, planes + 0, strides + 0, border, pic_w, pic_h);
    set_buf(&pr, planes + 3, strides + 2, pborder, pic_w, pic_h);
    return (int)warped_motion_prediction(&mvu, (uint16_t)pu[0], (uint16_t)pu[1], &cu, &g, &r0, &pr, (uint16_t)pu[2], (uint16_t)pu[3], &wm,
                                         (uint8_t)bit_depth, ASM_NON_AVX2);
}
