/*
 * tests/golden/ref_inter_pred_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own av1_inter_prediction and av1_inter_prediction_hbd (Codec/EbInterPrediction.c:1005, :2053) for
 * tests/golden/make_golden_inter_pred.py.  Contains no reference code: it builds the state the two functions read and calls them.
 *   - block geometry: the entry blk_geom_mds[0] (the reference's own table, Codec/EbUtility.c:614) filled the way md_scan_all_blks fills
 *     it (:750-775: bsize, bwidth / bheight, bwidth_uv = MAX(4, bwidth >> 1), bheight_uv, has_uv), cu_ptr->mds_idx = 0.  build_blk_geom
 *     itself cannot run in this build: it calls Log2f_SSE2, which exists only in the reference's NASM sources;
 *   - PictureControlSet_t: zeroed, with mi_grid_base (a ModeInfo grid with a margin, mi_stride = picture_width_in_sb * 16) and
 *     parent_pcs_ptr->sequence_control_set_ptr->picture_width_in_sb;
 *   - CodingUnit_t: mds_idx, av1xd (the four mb_to_*_edge values) and, for the 16-bit twin, interp_filters;
 *   - the neighbours of a sub-8x8 block as ModeInfo entries of the grid (ref_frame[0], mv[0]);
 *   - EbPictureBufferDesc_t for two references and the prediction (caller-owned padded planes).
 * The RTCD pointers the dispatch tables copy are set to the C kernels (no asm: the tables are filled by asmSetConvolve[Hbd]AsmTable).
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
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbUtility.h"

void asmSetConvolveAsmTable(void);
void asmSetConvolveHbdAsmTable(void);
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

/* own list of the block's own piece: av1_set_ref_frame(rf, ref_frame_type), rf[0] == LAST_FRAME ? 0 : 1 */
int drv_own_list(int ref_frame_type)
{
    MvReferenceFrame rf[2];
    av1_set_ref_frame(rf, (int8_t)ref_frame_type);
    return rf[0] == LAST_FRAME ? 0 : 1;
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

/* One call.  pu[] = pu_x, pu_y, dst_x, dst_y, bw, bh, bsize, interp_filters, ref_frame_type, pred_direction, mv0_row, mv0_col, mv1_row,
 * mv1_col, edge_left, edge_right, edge_top, edge_bottom, has_uv; nb[k] = (ref_frame0, mv_row, mv_col) for k = (row -1, col -1), (-1, 0), (0, -1).
 * pic_w: picture width (mi grid stride).  planes: ref0 Y/Cb/Cr, ref1 Y/Cb/Cr, pred Y/Cb/Cr; strides: luma / chroma of each; border: luma
 * padding of the references (origin_x = origin_y), pborder: of the prediction.  hbd: 16-bit planes and av1_inter_prediction_hbd. */
int drv_predict(int hbd, int bit_depth, const int32_t *pu, const int32_t *nb, int pic_w, int pic_h, void *const *planes, const int32_t *strides,
                int border, int pborder)
{
    static SequenceControlSet_t scs;
    static PictureParentControlSet_t ppcs;
    static PictureControlSet_t pcs;
    static CodingUnit_t cu;
    static MacroBlockD xd;
    memset(&scs, 0, sizeof(scs));
    memset(&ppcs, 0, sizeof(ppcs));
    memset(&pcs, 0, sizeof(pcs));
    memset(&cu, 0, sizeof(cu));
    memset(&xd, 0, sizeof(xd));
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
    if (hbd)
        av1_inter_prediction_hbd(&pcs, (uint8_t)pu[8], &cu, &mvu, (uint16_t)pu[0], (uint16_t)pu[1], (uint8_t)pu[4], (uint8_t)pu[5], &r0, &r1, &pr,
                                 (uint16_t)pu[2], (uint16_t)pu[3], (uint8_t)bit_depth, ASM_NON_AVX2);
    else
        av1_inter_prediction(&pcs, (uint32_t)pu[7], &cu, (uint8_t)pu[8], &mvu, (uint16_t)pu[0], (uint16_t)pu[1], (uint8_t)pu[4], (uint8_t)pu[5], &r0,
                             &r1, &pr, (uint16_t)pu[2], (uint16_t)pu[3], ASM_NON_AVX2);
    free(grid);
    free(mip);
    return 0;
}
