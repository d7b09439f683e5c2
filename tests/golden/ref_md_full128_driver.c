/*
 * tests/golden/ref_md_full128_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Runs the reference's own full-loop functions on one 128x128, 128x64 or 64x128 block for tests/golden/make_golden_md_full128.py and
 * tests/test_md_full128_vs_ref.py, with stand-in structs: zeroed allocations of the reference's own types in which only the fields those
 * functions read are set.  Contains no reference code, only calls into it:
 *   drv_md_full128_init       the rate tables of tests/golden/ref_coeff_rate_driver.c (av1_default_coef_probs, init_mode_probs,
 *                     av1_estimate_syntax_rate, av1_estimate_coefficients_rate), av1_build_quantizer into the parent picture set,
 *                     setup_rtcd_internal(ASM_NON_AVX2), and build_blk_geom(1): the BlockGeom of a block is the reference's own
 *                     (Codec/EbUtility.c:781-817), found in blk_geom_mds by its size at the superblock's origin
 *   drv_md_full128_full_loop  ProductFullLoop (Codec/EbFullLoop.c:946-1092), FullLoop_R (:1763-1920), CuFullDistortionFastTuMode_R (:1925-2083),
 *                     each whole, with its loop over txb_itr; then Av1InterFullCost / Av1IntraFullCost
 *                     (Codec/EbRateDistortionCost.c:1737-1840); then AV1PerformInverseTransformRecon (Codec/EbProductCodingLoop.c:885-1038)
 *                     with the has_coeff bits of the transform units filled from the candidate's masks, as product_full_mode_decision
 *                     fills them (Codec/EbModeDecision.c:2157-2184)
 * The residual the reference's ResidualKernel would leave is formed here by a plain subtraction.
 */
#define RTCD_C
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "EbDefinitions.h"
#include "aom_dsp_rtcd.h"
#include "EbCabacContextModel.h"
#include "EbCodingUnit.h"
#include "EbEntropyCoding.h"
#include "EbFullLoop.h"
#include "EbMdRateEstimation.h"
#include "EbModeDecision.h"
#include "EbModeDecisionProcess.h"
#include "EbPictureControlSet.h"
#include "EbRateDistortionCost.h"
#include "EbSequenceControlSet.h"
#include "EbUtility.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

void av1_build_quantizer(aom_bit_depth_t bit_depth, int32_t y_dc_delta_q, int32_t u_dc_delta_q, int32_t u_ac_delta_q, int32_t v_dc_delta_q,
                         int32_t v_ac_delta_q, Quants *const quants, Dequants *const deq);
void AV1PerformInverseTransformRecon(PictureControlSet_t *picture_control_set_ptr, ModeDecisionContext_t *context_ptr,
                                     ModeDecisionCandidateBuffer_t *candidateBuffer, CodingUnit_t *cu_ptr, const BlockGeom *blk_geom, EbAsm asm_type);

extern uint32_t max_num_active_blocks; /* Codec/EbUtility.c:606 */

/* build_blk_geom takes the logarithms of the block sides (bwidth_log2, which nothing here reads) with LOG2F, NASM code the link does not
 * have: a compiler builtin stands in, as in tests/golden/ref_cfl_driver.c */
uint32_t Log2f_SSE2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x | 1u); }

#define SB 128 /* the buffers of a candidate are superblock-sized: luma stride 128, chroma stride 64 */

static struct {
    MdRateEstimationContext_t *md;
    PictureControlSet_t *pcs;
    PictureParentControlSet_t *ppcs;
    SequenceControlSet_t *scs;
    EncodeContext_t *enc;
    EbObjectWrapper_t *wrap;
    ModeDecisionContext_t *ctx;
    ModeDecisionCandidateBuffer_t *buf;
    ModeDecisionCandidate_t *cand;
    CodingUnit_t *cu;
    EbTransQuantBuffers_t *tq;
    EbPictureBufferDesc_t *residual, *coeff, *quant, *recon_coeff, *pred, *recon;
    int geom_built;
} G;

static EbPictureBufferDesc_t *planes(size_t bytes_per_sample)
{
    EbPictureBufferDesc_t *p = (EbPictureBufferDesc_t *)calloc(1, sizeof(*p));
    p->bufferY = (EbByte)calloc(SB * SB, bytes_per_sample);
    p->bufferCb = (EbByte)calloc(SB * SB / 4, bytes_per_sample);
    p->bufferCr = (EbByte)calloc(SB * SB / 4, bytes_per_sample);
    p->strideY = SB, p->strideCb = p->strideCr = SB / 2;
    return p;
}

/* table_qindex: the base_qindex of the coefficient CDFs behind the rate tables; u / v deltas: those of av1_build_quantizer */
int drv_md_full128_init(int table_qindex, int chroma_delta_q)
{
    if (!G.md) {
        G.md = (MdRateEstimationContext_t *)calloc(1, sizeof(*G.md));
        G.pcs = (PictureControlSet_t *)calloc(1, sizeof(*G.pcs));
        G.ppcs = (PictureParentControlSet_t *)aligned_alloc(64, (sizeof(*G.ppcs) + 63) & ~(size_t)63);
        memset(G.ppcs, 0, sizeof(*G.ppcs));
        G.scs = (SequenceControlSet_t *)calloc(1, sizeof(*G.scs));
        G.enc = (EncodeContext_t *)calloc(1, sizeof(*G.enc));
        G.wrap = (EbObjectWrapper_t *)calloc(1, sizeof(*G.wrap));
        G.ctx = (ModeDecisionContext_t *)calloc(1, sizeof(*G.ctx));
        G.buf = (ModeDecisionCandidateBuffer_t *)calloc(1, sizeof(*G.buf));
        G.cand = (ModeDecisionCandidate_t *)calloc(1, sizeof(*G.cand));
        G.cu = (CodingUnit_t *)calloc(1, sizeof(*G.cu));
        G.tq = (EbTransQuantBuffers_t *)calloc(1, sizeof(*G.tq));
        G.residual = planes(2), G.coeff = planes(4), G.quant = planes(4), G.recon_coeff = planes(4), G.pred = planes(1), G.recon = planes(1);
        G.enc->asm_type = ASM_NON_AVX2;
        G.scs->encode_context_ptr = G.enc;
        G.wrap->objectPtr = G.scs;
        G.pcs->sequence_control_set_wrapper_ptr = G.wrap;
        G.pcs->parent_pcs_ptr = G.ppcs;
        G.tq->tuTransCoeff2Nx2NPtr = G.coeff;
        G.ctx->trans_quant_buffers_ptr = G.tq;
        G.ctx->transform_inner_array_ptr = (int16_t *)calloc(SB * SB, sizeof(int16_t));
        G.ctx->cu_ptr = G.cu;
        G.buf->candidate_ptr = G.cand;
        G.buf->residual_ptr = G.residual, G.buf->residualQuantCoeffPtr = G.quant, G.buf->reconCoeffPtr = G.recon_coeff;
        G.buf->prediction_ptr = G.pred, G.buf->reconPtr = G.recon;
        G.cand->md_rate_estimation_ptr = G.md;
    }
    FRAME_CONTEXT *fc = (FRAME_CONTEXT *)calloc(1, sizeof(FRAME_CONTEXT));
    if (!fc) return -1;
    memset(G.md, 0, sizeof(*G.md));
    av1_default_coef_probs(fc, table_qindex);
    init_mode_probs(fc);
    av1_estimate_syntax_rate(G.md, EB_FALSE, fc);
    av1_estimate_coefficients_rate(G.md, fc);
    free(fc);
    av1_build_quantizer(AOM_BITS_8, 0, chroma_delta_q, chroma_delta_q, chroma_delta_q, chroma_delta_q, &G.ppcs->quants, &G.ppcs->deq);
    av1_build_quantizer(AOM_BITS_8, 0, chroma_delta_q, chroma_delta_q, chroma_delta_q, chroma_delta_q, &G.ppcs->quantsMd, &G.ppcs->deqMd);
    setup_rtcd_internal(ASM_NON_AVX2);
    if (!G.geom_built) build_blk_geom(1), G.geom_built = 1;
    return 0;
}

/* the reference's geometry of the w x h block at the origin of a 128x128 superblock: txb_count and tx_org[4][2] for the caller to see */
static const BlockGeom *geom_of(int w, int h)
{
    for (uint32_t i = 0; i < max_num_active_blocks; i++) {
        const BlockGeom *g = Get_blk_geom_mds(i);
        if (g->bwidth == w && g->bheight == h && g->origin_x == 0 && g->origin_y == 0) return g;
    }
    return NULL;
}

int drv_md_full128_geometry(int w, int h, int32_t *txb_count, int32_t *tx_org /* [4][2] */, int32_t *tx_sizes /* [2]: txsize[0], txsize_uv[0] */)
{
    const BlockGeom *g = geom_of(w, h);
    if (!g) return -1;
    *txb_count = g->txb_count;
    for (int t = 0; t < g->txb_count && t < 4; t++) tx_org[2 * t] = g->tx_org_x[t], tx_org[2 * t + 1] = g->tx_org_y[t];
    tx_sizes[0] = g->txsize[0], tx_sizes[1] = g->txsize_uv[0];
    return 0;
}

/* src / pred: the block's Y, Cb, Cr (8-bit) with their strides.  in[]: qindex, is_inter, merge_flag, intra_mode, tx_type_y, tx_type_uv,
 * txb_skip_ctx[3], dc_sign_ctx[3], skip_flag_context, reduced_tx_set, skipModeFacBits[skip_flag_context][1].  rates[]: fast_luma_rate, fast_chroma_rate, lambda.
 * out64[]: y_dist[2], cb_dist[2], cr_dist[2], bits[3], full cost, merge cost, skip cost, full_lambda_rate, full_cost_luma, the last TU's
 * three_quad_energy.  out32[]: eob[3][4], quantized_dc[3], y_, u_, v_has_coeff, skip_flag (block_has_coeff is assigned by AV1PerformFullLoop
 * itself, EbProductCodingLoop.c:2229, which is not run).  recon: Y w x h, Cb, Cr
 * tightly packed one after the other. */
int drv_md_full128_full_loop(int w, int h, const uint8_t *const src[3], const int32_t src_stride[3], const uint8_t *const pred[3], const int32_t pred_stride[3],
                     const int32_t *in, const uint64_t *rates, uint64_t *out64, int32_t *out32, uint8_t *recon)
{
    const BlockGeom *g = geom_of(w, h);
    if (!g || !G.md) return -1;
    ModeDecisionCandidate_t *cand = G.cand;
    MdRateEstimationContext_t *md = cand->md_rate_estimation_ptr;
    memset(cand, 0, sizeof(*cand));
    cand->md_rate_estimation_ptr = md;
    memset(G.cu, 0, sizeof(*G.cu));
    const int qindex = in[0], is_inter = in[1], merge = in[2];
    cand->type = is_inter ? INTER_MODE : INTRA_MODE;
    cand->merge_flag = merge ? EB_TRUE : EB_FALSE;
    cand->pred_mode = (PredictionMode)in[3];
    cand->intra_chroma_mode = UV_DC_PRED;
    cand->transform_type[PLANE_TYPE_Y] = (TxType)in[4], cand->transform_type[PLANE_TYPE_UV] = (TxType)in[5];
    cand->fast_luma_rate = rates[0], cand->fast_chroma_rate = rates[1];
    G.cu->luma_txb_skip_context = (int16_t)in[6], G.cu->cb_txb_skip_context = (int16_t)in[7], G.cu->cr_txb_skip_context = (int16_t)in[8];
    G.cu->luma_dc_sign_context = (int16_t)in[9], G.cu->cb_dc_sign_context = (int16_t)in[10], G.cu->cr_dc_sign_context = (int16_t)in[11];
    G.cu->skip_flag_context = (unsigned)in[12];
    G.ppcs->reduced_tx_set_used = in[13];
    md->skipModeFacBits[in[12]][1] = in[14];   /* the one skip-mode entry Av1MergeSkipFullCost reads: the caller's skip_mode_rate */
    G.ppcs->base_qindex = (uint8_t)qindex;
    G.ctx->blk_geom = g;
    G.ctx->full_lambda = (uint32_t)rates[2];
    if (G.ctx->full_lambda != rates[2]) return -2;
    for (int p = 0; p < 3; p++) {
        const int pw = p ? w / 2 : w, ph = p ? h / 2 : h, stride = p ? SB / 2 : SB;
        int16_t *res = (int16_t *)(p == 0 ? G.residual->bufferY : p == 1 ? G.residual->bufferCb : G.residual->bufferCr);
        uint8_t *pr = p == 0 ? G.pred->bufferY : p == 1 ? G.pred->bufferCb : G.pred->bufferCr;
        for (int y = 0; y < ph; y++)
            for (int x = 0; x < pw; x++) {
                pr[y * stride + x] = pred[p][y * pred_stride[p] + x];
                res[y * stride + x] = (int16_t)((int)src[p][y * src_stride[p] + x] - (int)pred[p][y * pred_stride[p] + x]);
            }
    }
    uint32_t count[3][MAX_NUM_OF_TU_PER_CU];
    memset(count, 0, sizeof(count));
    uint64_t y_dist[DIST_CALC_TOTAL] = {0, 0}, cb_dist[DIST_CALC_TOTAL] = {0, 0}, cr_dist[DIST_CALC_TOTAL] = {0, 0};
    uint64_t y_bits = 0, cb_bits = 0, cr_bits = 0;
    ProductFullLoop(G.buf, G.ctx, G.pcs, (uint32_t)qindex, count[0], &y_bits, y_dist);
    const uint64_t energy = G.ctx->three_quad_energy;
    FullLoop_R(NULL, G.buf, G.ctx, NULL, G.pcs, PICTURE_BUFFER_DESC_CHROMA_MASK, (uint32_t)qindex, (uint32_t)qindex, count[1], count[2]);
    CuFullDistortionFastTuMode_R(NULL, G.buf, G.ctx, cand, G.pcs, cb_dist, cr_dist, count, COMPONENT_CHROMA, &cb_bits, &cr_bits, ASM_NON_AVX2);
    out64[0] = y_dist[0], out64[1] = y_dist[1], out64[2] = cb_dist[0], out64[3] = cb_dist[1], out64[4] = cr_dist[0], out64[5] = cr_dist[1];
    out64[6] = y_bits, out64[7] = cb_bits, out64[8] = cr_bits;
    for (int p = 0; p < 3; p++) {
        for (int t = 0; t < 4; t++) out32[4 * p + t] = t < g->txb_count ? cand->eob[p][t] : 0;
        out32[12 + p] = cand->quantized_dc[p];
    }
    out32[15] = cand->y_has_coeff, out32[16] = cand->u_has_coeff, out32[17] = cand->v_has_coeff;
    uint64_t cost = 0, merge_cost = 0, skip_cost = 0;
    G.buf->full_cost_ptr = &cost, G.buf->full_cost_merge_ptr = &merge_cost, G.buf->full_cost_skip_ptr = &skip_cost;
    G.buf->full_lambda_rate = G.buf->full_cost_luma = 0;
    const EbErrorType rc = is_inter ? Av1InterFullCost(G.pcs, G.ctx, G.buf, G.cu, y_dist, cb_dist, cr_dist, rates[2], &y_bits, &cb_bits, &cr_bits, g->bsize)
                                    : Av1IntraFullCost(G.pcs, G.ctx, G.buf, G.cu, y_dist, cb_dist, cr_dist, rates[2], &y_bits, &cb_bits, &cr_bits, g->bsize);
    out64[9] = cost, out64[10] = merge_cost, out64[11] = skip_cost, out64[12] = G.buf->full_lambda_rate, out64[13] = G.buf->full_cost_luma, out64[14] = energy;
    out32[18] = cand->skip_flag;
    /* the host's fill of the transform units (EbModeDecision.c:2157-2184), then the reconstruction */
    for (int t = 0; t < g->txb_count; t++) {
        G.cu->transform_unit_array[t].y_has_coeff = (cand->y_has_coeff >> t) & 1;
        G.cu->transform_unit_array[t].u_has_coeff = (cand->u_has_coeff >> t) & 1;
        G.cu->transform_unit_array[t].v_has_coeff = (cand->v_has_coeff >> t) & 1;
    }
    G.pcs->intra_md_open_loop_flag = EB_FALSE;
    memset(G.recon->bufferY, 0, SB * SB), memset(G.recon->bufferCb, 0, SB * SB / 4), memset(G.recon->bufferCr, 0, SB * SB / 4);
    AV1PerformInverseTransformRecon(G.pcs, G.ctx, G.buf, G.cu, g, ASM_NON_AVX2);
    for (int p = 0; p < 3; p++) {
        const int pw = p ? w / 2 : w, ph = p ? h / 2 : h, stride = p ? SB / 2 : SB;
        const uint8_t *r = p == 0 ? G.recon->bufferY : p == 1 ? G.recon->bufferCb : G.recon->bufferCr;
        for (int y = 0; y < ph; y++) memcpy(recon, r + y * stride, (size_t)pw), recon += pw;
    }
    return rc == EB_ErrorNone ? 0 : -3;
}
