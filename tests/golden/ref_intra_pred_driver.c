/*
 * tests/golden/ref_intra_pred_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own intra prediction for tests/golden/make_golden_intra_pred.py and tests/test_intra_pred_vs_ref.py.  Contains no
 * reference code: it reaches the statics build_intra_predictors, build_intra_predictors_high, has_top_right and has_bottom_left by
 * including the reference's EbIntraPrediction.c (its object is left out of the link, the way oracle/ref_subpel_search_driver.c reaches
 * the ME statics), binds the per-size RTCD predictor pointers to the reference's C bodies, and runs the reference's two table
 * initialisers.  The reference has no PAETH predictor (pred[PAETH_PRED] is never assigned, highbd_paeth_predictor is commented out), so
 * mode 12 must not be passed.
 *   drv_build      one call of build_intra_predictors (ED_STAGE) / build_intra_predictors_high with the given edges, counts, mode;
 *   drv_position   av1_predict_intra_block (ED_STAGE, luma; bit_depth 8) or av1_predict_intra_block_16bit (bit_depth 10) for a block at a
 *                  picture position, reading the edges from neighbour arrays the caller filled, and the four counts of that position:
 *                  has_top_right / has_bottom_left are the reference's own functions, called with the arguments
 *                  av1_predict_intra_block gives them.  The caller runs every position with V, H, D45 and D203, which between them read
 *                  every sample the four counts admit, and checks drv_build with these counts against the block written here: a wrong
 *                  count cannot pass.
 *   drv_md         the mode-decision sequence for the same position: generate_intra_reference_samples on a ModeDecisionContext_t whose
 *                  luma recon neighbour array holds the same edge samples, then av1_predict_intra_block(MD_STAGE).
 */
#define RTCD_C
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "EbIntraPrediction.c"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbEncDecProcess.h"
#include "EbModeDecisionProcess.h"
#include "EbNeighborArrays.h"

#define BIND1(t, bw, bh)                                                         \
    aom_##t##_predictor_##bw##x##bh = aom_##t##_predictor_##bw##x##bh##_c;       \
    aom_highbd_##t##_predictor_##bw##x##bh = aom_highbd_##t##_predictor_##bw##x##bh##_c;
#define BIND(bw, bh)                                                                                                                 \
    BIND1(dc, bw, bh) BIND1(dc_top, bw, bh) BIND1(dc_left, bw, bh) BIND1(dc_128, bw, bh) BIND1(v, bw, bh) BIND1(h, bw, bh)            \
    BIND1(smooth, bw, bh) BIND1(smooth_v, bw, bh) BIND1(smooth_h, bw, bh)

int drv_init(void)
{
    BIND(4, 4) BIND(8, 8) BIND(16, 16) BIND(32, 32) BIND(64, 64) BIND(4, 8) BIND(8, 4) BIND(8, 16) BIND(16, 8) BIND(16, 32) BIND(32, 16)
    BIND(32, 64) BIND(64, 32) BIND(4, 16) BIND(16, 4) BIND(8, 32) BIND(32, 8) BIND(16, 64) BIND(64, 16)
    av1_dr_prediction_z1 = av1_dr_prediction_z1_c;
    av1_dr_prediction_z2 = av1_dr_prediction_z2_c;
    av1_dr_prediction_z3 = av1_dr_prediction_z3_c;
    av1_highbd_dr_prediction_z1 = av1_highbd_dr_prediction_z1_c;
    av1_highbd_dr_prediction_z2 = av1_highbd_dr_prediction_z2_c;
    av1_highbd_dr_prediction_z3 = av1_highbd_dr_prediction_z3_c;
    init_intra_dc_predictors_c_internal();
    init_intra_predictors_internal();
    return 0;
}

/* above / left: the caller's arrays with sample -1 at index 0 (above_ref = above + 1); counts[4] = n_top_px, n_topright_px, n_left_px,
 * n_bottomleft_px; dst: tx block with stride dst_stride, in samples of the depth */
int drv_build(int bit_depth, void *above, void *left, void *dst, int dst_stride, int mode, int angle_delta, int tx_size, const int32_t *counts)
{
    if (bit_depth == 8)
        build_intra_predictors(NULL, ED_STAGE, DC_PRED, DC_PRED, DC_PRED, DC_PRED, (uint8_t *)above + 1, (uint8_t *)left + 1, (uint8_t *)dst,
                               dst_stride, (PredictionMode)mode, angle_delta, FILTER_INTRA_MODES, (TxSize)tx_size, 1, counts[0], counts[1],
                               counts[2], counts[3], 0);
    else
        build_intra_predictors_high(NULL, NULL, (uint16_t *)above + 1, (uint16_t *)left + 1, (uint16_t *)dst, dst_stride, (PredictionMode)mode,
                                    angle_delta, FILTER_INTRA_MODES, (TxSize)tx_size, 1, counts[0], counts[1], counts[2], counts[3], 0,
                                    bit_depth);
    return 0;
}

static int find_bsize(int w, int h)
{
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == w && block_size_high[b] == h) return b;
    return -1;
}

static int find_txsize(int w, int h)
{
    for (int t = 0; t < TX_SIZES_ALL; t++)
        if (tx_size_wide[t] == w && tx_size_high[t] == h) return t;
    return -1;
}

/* A luma block of w x h (one transform block of the same size) with partition shape `shape` at picture sample (x, y) of a pic_w x pic_h
 * picture: av1_predict_intra_block(ED_STAGE) into recon (pic_h rows of `stride` bytes, origin 0) and the four counts of that position. */
static void fill_common(Av1Common *cm, BlockGeom *g, int w, int h, int shape, int bsize, int tx, int pic_w, int pic_h)
{
    memset(cm, 0, sizeof(*cm));
    cm->mi_cols = ((pic_w + 7) >> 3) << 1;
    cm->mi_rows = ((pic_h + 7) >> 3) << 1;
    /* has_top_right / has_bottom_left read the superblock size through the picture's control sets: 64x64, as the reference sets it */
    static PictureParentControlSet_t *pcs;
    if (!pcs) {
        pcs = (PictureParentControlSet_t *)calloc(1, sizeof(*pcs));
        pcs->sequence_control_set_ptr = (SequenceControlSet_t *)calloc(1, sizeof(SequenceControlSet_t));
        pcs->sequence_control_set_ptr->sb_size = BLOCK_64X64;
    }
    cm->p_pcs_ptr = pcs;
    memset(g, 0, sizeof(*g));
    g->shape = (PART)shape;
    g->bsize = (BlockSize)bsize;
    g->bwidth = (uint8_t)w;
    g->bheight = (uint8_t)h;
    g->txsize[0] = (TxSize)tx;
}

int drv_position(int bit_depth, int w, int h, int shape, int x, int y, int pic_w, int pic_h, int mode, int angle_delta, void *above, void *left,
                 void *recon, int stride, int32_t *counts)
{
    const int bsize = find_bsize(w, h), tx = find_txsize(w, h);
    if (bsize < 0 || tx < 0) return -1;
    Av1Common cm;
    BlockGeom g;
    fill_common(&cm, &g, w, h, shape, bsize, tx, pic_w, pic_h);
    EbPictureBufferDesc_t rb;
    memset(&rb, 0, sizeof(rb));
    rb.bufferY = (EbByte)recon;
    rb.strideY = (uint16_t)stride;
    if (bit_depth == 8) {
        av1_predict_intra_block(NULL, ED_STAGE, DC_PRED, DC_PRED, DC_PRED, DC_PRED, &g, &cm, w, h, (TxSize)tx, (PredictionMode)mode, angle_delta,
                                0, FILTER_INTRA_MODES, (uint8_t *)above + 1, (uint8_t *)left + 1, &rb, 0, (BlockSize)bsize, (uint32_t)x,
                                (uint32_t)y, 0, 0);
    } else {
        static EncDecContext_t *ed;
        if (!ed) ed = (EncDecContext_t *)calloc(1, sizeof(*ed));
        ed->blk_geom = &g;
        av1_predict_intra_block_16bit(ed, NULL, &cm, w, h, (TxSize)tx, (PredictionMode)mode, angle_delta, 0, FILTER_INTRA_MODES,
                                      (uint16_t *)above + 1, (uint16_t *)left + 1, &rb, 0, 0, 0, (BlockSize)bsize, (uint32_t)x, (uint32_t)y);
    }

    /* the counts: the reference's availability functions on the arguments av1_predict_intra_block (:9739-9833) gives them */
    const int mirow = y >> 2, micol = x >> 2;
    const int have_top = mirow > 0, have_left = micol > 0;
    const int mb_to_bottom_edge = ((cm.mi_rows - mi_size_high[bsize] - mirow) * MI_SIZE) * 8;
    const int mb_to_right_edge = ((cm.mi_cols - mi_size_wide[bsize] - micol) * MI_SIZE) * 8;
    const int xr = (mb_to_right_edge >> 3), yd = (mb_to_bottom_edge >> 3);
    const int right_available = micol + tx_size_wide_unit[tx] < cm.mi_cols;
    const int bottom_available = (yd > 0) && (mirow + tx_size_high_unit[tx] < cm.mi_rows);
    const PartitionType partition = from_shape_to_part[shape];
    const int htr = has_top_right(&cm, (BlockSize)bsize, mirow, micol, have_top, right_available, partition, (TxSize)tx, 0, 0, 0, 0);
    const int hbl = has_bottom_left(&cm, (BlockSize)bsize, mirow, micol, bottom_available, have_left, partition, (TxSize)tx, 0, 0, 0, 0);
    counts[0] = have_top ? AOMMIN(w, xr + w) : 0;
    counts[1] = htr ? AOMMIN(w, xr) : 0;
    counts[2] = have_left ? AOMMIN(h, yd + h) : 0;
    counts[3] = hbl ? AOMMIN(h, yd) : 0;
    return 0;
}

static NeighborArrayUnit_t *new_unit(int size, int log2)
{
    NeighborArrayUnit_t *u = (NeighborArrayUnit_t *)calloc(1, sizeof(*u));
    u->leftArray = (uint8_t *)calloc(1, size);
    u->topArray = (uint8_t *)calloc(1, size);
    u->topLeftArray = (uint8_t *)calloc(1, 2 * MAX_PICTURE_HEIGHT_SIZE + size);
    u->unitSize = 1;
    u->granularityNormalLog2 = u->granularityTopLeftLog2 = (uint8_t)log2;
    u->granularityNormal = u->granularityTopLeft = (uint8_t)(1 << log2);
    return u;
}

/* The mode-decision sequence (8 bits, luma) for the block drv_position predicts: above[0] / left[0] = sample -1, above[1 ..] / left[1 ..]
 * 2 w / 2 h edge samples, laid into the luma recon neighbour array at the block's position; dst: w x h, stride w. */
int drv_md(int w, int h, int shape, int x, int y, int pic_w, int pic_h, int mode, int angle_delta, const uint8_t *above, const uint8_t *left,
           uint8_t *dst)
{
    const int bsize = find_bsize(w, h), tx = find_txsize(w, h);
    if (bsize < 0 || tx < 0) return -1;
    Av1Common cm;
    BlockGeom g;
    fill_common(&cm, &g, w, h, shape, bsize, tx, pic_w, pic_h);
    static ModeDecisionContext_t *md;
    if (!md) {
        md = (ModeDecisionContext_t *)calloc(1, sizeof(*md));
        md->mode_type_neighbor_array = new_unit(4096, 2);
        md->intra_luma_mode_neighbor_array = new_unit(4096, 2);
        md->intra_chroma_mode_neighbor_array = new_unit(4096, 2);
        md->luma_recon_neighbor_array = new_unit(4096, 0);
    }
    md->blk_geom = &g;
    md->cu_origin_x = (uint16_t)x;
    md->cu_origin_y = (uint16_t)y;
    md->round_origin_x = (uint32_t)((x >> 3) << 3);
    md->round_origin_y = (uint32_t)((y >> 3) << 3);
    NeighborArrayUnit_t *u = md->luma_recon_neighbor_array;
    memcpy(u->topArray + x, above + 1, 2 * w);
    memcpy(u->leftArray + y, left + 1, 2 * h);
    u->topLeftArray[MAX_PICTURE_HEIGHT_SIZE + x - y] = above[0];
    generate_intra_reference_samples(&cm, md);
    EbPictureBufferDesc_t rb;
    memset(&rb, 0, sizeof(rb));
    rb.bufferY = dst;
    rb.strideY = (uint16_t)w;
    av1_predict_intra_block(md, MD_STAGE, DC_PRED, DC_PRED, DC_PRED, DC_PRED, &g, &cm, w, h, (TxSize)tx, (PredictionMode)mode, angle_delta, 0,
                            FILTER_INTRA_MODES, NULL, NULL, &rb, 0, (BlockSize)bsize, (uint32_t)x, (uint32_t)y, 0, 0);
    return 0;
}
