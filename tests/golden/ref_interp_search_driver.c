/*
 * tests/golden/ref_interp_search_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own interpolation-filter search and the pieces under it (Codec/EbInterPrediction.c) for
 * tests/golden/make_golden_md_ifs.py, tests/test_md_ifs_vs_ref.py and tools/md_ifs_probe.py.  Contains no reference code: it builds the
 * state the functions read and calls them.
 *   drv_ifs_variance64     highbd_variance64_c (:3161) or highbd_variance64_avx2 (ASM_AVX2/variance_avx2.c:325) on 8-bit pointers; returns sse
 *   drv_ifs_lapndz         av1_model_rd_from_var_lapndz (:3314)
 *   drv_ifs_from_sse       model_rd_from_sse (:3339)
 *   drv_ifs_max_quantizer  av1_ac_quant_Q3(255, 0, AOM_BITS_8): the largest y_dequant_Q3[.][1] of 8-bit video
 *   drv_ifs_search         interpolation_filter_search (:3523) itself, on
 *     - PictureControlSet_t / PictureParentControlSet_t / SequenceControlSet_t, zeroed, with the fields the function and its callees
 *       read: av1_cm->interp_filter = SWITCHABLE, interpolation_filter_search_mode, enable_dual_filter, base_qindex and
 *       deq.y_dequant_Q3[base_qindex][1], enhanced_picture_ptr (the source, its origin the block's position), the mi grid and
 *       picture_width_in_sb as tests/golden/ref_inter_pred_driver.c builds them;
 *     - ModeDecisionContext_t, zeroed: cu_origin = (0, 0) -- so av1_get_pred_context_switchable_interp reads no neighbour and returns
 *       SWITCHABLE_FILTERS (+ 4 for a compound candidate, + 8 for dir 1) -- with the two rows of switchable_interp_FacBitss at those
 *       contexts set to the caller's filter_rate, full_lambda, blk_geom (blk_geom_mds[0] filled as md_scan_all_blks fills it) and cu_ptr;
 *     - the reference and prediction planes as EbPictureBufferDesc_t; the caller points the reference planes at the block, since
 *       cu_origin is (0, 0).
 */
#define RTCD_C
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "EbDefinitions.h"
#include "aom_dsp_rtcd.h"
#include "EbCodingUnit.h"
#include "EbInterPrediction.h"
#include "EbMdRateEstimation.h"
#include "EbModeDecision.h"
#include "EbModeDecisionProcess.h"
#include "EbNeighborArrays.h"
#include "EbPictureBufferDesc.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbUtility.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

void asmSetConvolveAsmTable(void);
void asmSetConvolveHbdAsmTable(void);
extern BlockGeom blk_geom_mds[];
int16_t av1_ac_quant_Q3(int32_t qindex, int32_t delta, aom_bit_depth_t bit_depth);
void av1_model_rd_from_var_lapndz(int64_t var, uint32_t n_log2, uint32_t qstep, int32_t *rate, int64_t *dist);
void model_rd_from_sse(BlockSize bsize, int16_t quantizer, int64_t sse, int32_t *rate, int64_t *dist);
void interpolation_filter_search(PictureControlSet_t *picture_control_set_ptr, EbPictureBufferDesc_t *prediction_ptr,
                                 ModeDecisionContext_t *md_context_ptr, ModeDecisionCandidateBuffer_t *candidate_buffer_ptr, MvUnit_t mv_unit,
                                 EbPictureBufferDesc_t *ref_pic_list0, EbPictureBufferDesc_t *ref_pic_list1, EbAsm asm_type, int64_t *const rd,
                                 int32_t *const switchable_rate, int32_t *const skip_txfm_sb, int64_t *const skip_sse_sb);

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
    highbd_variance64 = highbd_variance64_c;
    asmSetConvolveAsmTable();
    return 0;
}

uint64_t drv_ifs_variance64(int avx2, const uint8_t *a, int32_t a_stride, const uint8_t *b, int32_t b_stride, int32_t w, int32_t h)
{
    uint64_t sse = 0;
    int64_t sum = 0;
    (avx2 ? highbd_variance64_avx2 : highbd_variance64_c)(a, a_stride, b, b_stride, w, h, &sse, &sum);
    return sse;
}

void drv_ifs_lapndz(int64_t var, uint32_t n_log2, uint32_t qstep, int32_t *rate, int64_t *dist)
{
    av1_model_rd_from_var_lapndz(var, n_log2, qstep, rate, dist);
}

void drv_ifs_from_sse(int bsize, int quantizer, int64_t sse, int32_t *rate, int64_t *dist)
{
    model_rd_from_sse((BlockSize)bsize, (int16_t)quantizer, sse, rate, dist);
}

int drv_ifs_max_quantizer(void) { return av1_ac_quant_Q3(255, 0, AOM_BITS_8); }

static void set_buf(EbPictureBufferDesc_t *b, void *const planes[3], const int32_t strides[2], int origin_x, int origin_y)
{
    memset(b, 0, sizeof(*b));
    b->bufferY = (EbByte)planes[0];
    b->bufferCb = (EbByte)planes[1];
    b->bufferCr = (EbByte)planes[2];
    b->strideY = (uint16_t)strides[0];
    b->strideCb = b->strideCr = (uint16_t)strides[1];
    b->origin_x = (uint16_t)origin_x;
    b->origin_y = (uint16_t)origin_y;
}

/* One candidate.  pu[] = bw, bh, bsize, bsize_uv, ref_frame_type, pred_direction, mv0_row, mv0_col, mv1_row, mv1_col, edge_left, edge_right,
 * edge_top, edge_bottom, src_x, src_y, quantizer, search_mode, enable_dual_filter; filter_rate[2][3]; planes: ref0 Y/Cb/Cr, ref1
 * Y/Cb/Cr (each pointing border samples above and left of the block), the source Y/Cb/Cr at sample (0, 0), the prediction tile Y/Cb/Cr;
 * strides: luma / chroma of each of the four.  out[] = interp_filters, switchable_rate, rd, skip_sse_sb, skip_txfm_sb.
 * `repeat` calls the function that many times (the probe's timing loop). */
int drv_ifs_search(const int32_t *pu, const int32_t *filter_rate, uint32_t full_lambda, void *const *planes, const int32_t *strides, int border,
                   int64_t *out, int repeat)
{
    static SequenceControlSet_t scs;
    static PictureParentControlSet_t ppcs;
    static PictureControlSet_t pcs;
    static Av1Common cm;
    static ModeDecisionContext_t md;
    static MdRateEstimationContext_t rates;
    static NeighborArrayUnit_t rf_na;
    static NeighborArrayUnit32_t it_na;
    static ModeDecisionCandidateBuffer_t buffer;
    static ModeDecisionCandidate_t cand;
    static CodingUnit_t cu;
    static MacroBlockD xd;
    memset(&scs, 0, sizeof(scs)), memset(&ppcs, 0, sizeof(ppcs)), memset(&pcs, 0, sizeof(pcs)), memset(&cm, 0, sizeof(cm));
    memset(&md, 0, sizeof(md)), memset(&rates, 0, sizeof(rates)), memset(&rf_na, 0, sizeof(rf_na)), memset(&it_na, 0, sizeof(it_na));
    memset(&buffer, 0, sizeof(buffer)), memset(&cand, 0, sizeof(cand)), memset(&cu, 0, sizeof(cu)), memset(&xd, 0, sizeof(xd));
    const int bw = pu[0], bh = pu[1], compound = pu[5] == 2;

    scs.picture_width_in_sb = 4;
    scs.enable_dual_filter = (uint8_t)pu[18];
    ppcs.sequence_control_set_ptr = &scs;
    ppcs.av1_cm = &cm;
    cm.interp_filter = SWITCHABLE;
    ppcs.interpolation_filter_search_mode = (uint8_t)pu[17];
    ppcs.base_qindex = 100;
    ppcs.deq.y_dequant_Q3[100][1] = (int16_t)pu[16];
    pcs.parent_pcs_ptr = &ppcs;
    const int stride = scs.picture_width_in_sb * 16, rows = 64, margin = stride + 1;
    ModeInfo *mip = (ModeInfo *)calloc((size_t)(rows + 2) * stride + 2, sizeof(ModeInfo));
    ModeInfo **grid = (ModeInfo **)calloc((size_t)rows * stride, sizeof(ModeInfo *));
    if (!mip || !grid) return -1;
    for (size_t i = 0; i < (size_t)rows * stride; i++) grid[i] = mip + margin + i;
    pcs.mi_grid_base = grid;

    EbPictureBufferDesc_t r0, r1, src, pr;
    set_buf(&r0, planes + 0, strides + 0, border, border);
    set_buf(&r1, planes + 3, strides + 2, border, border);
    set_buf(&src, planes + 6, strides + 4, pu[14], pu[15]);
    set_buf(&pr, planes + 9, strides + 6, 0, 0);
    ppcs.enhanced_picture_ptr = &src;

    BlockGeom *g = &blk_geom_mds[0];
    memset(g, 0, sizeof(*g));
    g->bsize = (BlockSize)pu[2];
    g->bsize_uv = (BlockSize)pu[3];
    g->bwidth = (uint8_t)bw;
    g->bheight = (uint8_t)bh;
    g->bwidth_uv = (uint8_t)(bw >> 1 > 4 ? bw >> 1 : 4);
    g->bheight_uv = (uint8_t)(bh >> 1 > 4 ? bh >> 1 : 4);
    g->has_uv = 1;
    xd.mb_to_left_edge = pu[10];
    xd.mb_to_right_edge = pu[11];
    xd.mb_to_top_edge = pu[12];
    xd.mb_to_bottom_edge = pu[13];
    cu.av1xd = &xd;
    cu.mds_idx = 0;

    const int ctx0 = SWITCHABLE_FILTERS + (compound ? SWITCHABLE_FILTERS + 1 : 0), ctx1 = ctx0 + 2 * (SWITCHABLE_FILTERS + 1);
    for (int f = 0; f < SWITCHABLE_FILTERS; f++) {
        rates.switchable_interp_FacBitss[ctx0][f] = filter_rate[f];
        rates.switchable_interp_FacBitss[ctx1][f] = filter_rate[3 + f];
    }
    md.md_rate_estimation_ptr = &rates;
    md.ref_frame_type_neighbor_array = &rf_na;
    md.interpolation_type_neighbor_array = &it_na;
    md.full_lambda = full_lambda;
    md.cu_ptr = &cu;
    md.blk_geom = g;
    md.cu_origin_x = md.cu_origin_y = 0;

    cand.ref_frame_type = (uint8_t)pu[4];
    cand.is_compound = (EbBool)compound;
    cand.pred_mode = NEWMV;
    cand.motion_mode = SIMPLE_TRANSLATION;
    cand.merge_flag = EB_FALSE;
    buffer.candidate_ptr = &cand;

    MvUnit_t mvu;
    memset(&mvu, 0, sizeof(mvu));
    mvu.predDirection = (uint8_t)pu[5];
    mvu.mv[0].y = (int16_t)pu[6];
    mvu.mv[0].x = (int16_t)pu[7];
    mvu.mv[1].y = (int16_t)pu[8];
    mvu.mv[1].x = (int16_t)pu[9];

    int64_t rd = 0, skip_sse = 0;
    int32_t rs = 0, skip = 0;
    for (int k = 0; k < (repeat > 0 ? repeat : 1); k++)
        interpolation_filter_search(&pcs, &pr, &md, &buffer, mvu, &r0, &r1, ASM_NON_AVX2, &rd, &rs, &skip, &skip_sse);
    out[0] = cand.interp_filters, out[1] = rs, out[2] = rd, out[3] = skip_sse, out[4] = skip;
    free(grid);
    free(mip);
    return 0;
}
