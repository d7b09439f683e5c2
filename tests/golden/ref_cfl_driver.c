/*
 * tests/golden/ref_cfl_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own chroma-from-luma functions for tests/golden/make_golden_cfl.py and tests/test_cfl_vs_ref.py.  Contains no
 * reference code: it reaches the static cfl_rd_pick_alpha by including the reference's EbProductCodingLoop.c (its object is left out of
 * the link, the way tests/golden/ref_intra_pred_driver.c reaches the intra statics).
 *   drv_subsample         cfl_luma_subsampling_420_lbd_c / _hbd_c into a CFL_BUF_LINE x CFL_BUF_LINE buffer
 *   drv_subtract_average  subtract_average_c or subtract_average_avx2, with the arguments CflPrediction gives them (its LOG2F is NASM code the link
 *                         does not have: the two logarithms are taken with a compiler builtin)
 *   drv_predict           cfl_predict_lbd_c / _hbd_c or their AVX2 forms
 *   drv_idx_to_alpha      cfl_idx_to_alpha
 *   drv_pick_alpha        cfl_rd_pick_alpha itself on contexts that hold only what it and AV1CostCalcCfl read.  FullLoop_R and
 *                         CuFullDistortionFastTuMode_R below take the place of the reference's (the generator weakens those two symbols of
 *                         EbFullLoop.o), and the RTCD pointers cfl_predict_lbd and ResidualKernel point at the two hooks below.  The
 *                         prediction hook notes the alpha_q3 AV1CostCalcCfl asks a prediction for -- the candidate the reference
 *                         evaluates, whatever (cfl_alpha_idx, cfl_alpha_signs) it was derived from -- and the distortion stand-in answers
 *                         with that candidate's bits and distortion from the caller's tables and records it in the plane's mask.
 */
#define RTCD_C
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "EbProductCodingLoop.c"
#include "aom_dsp_rtcd.h"
#include "EbIntraPrediction.h"
#include "EbMdRateEstimation.h"

static struct {
    const uint64_t *bits, *dist;   /* [2][33] each */
    uint64_t mask[2];
    int alpha_q3;
    int n_keys;
    int32_t keys[256][4];          /* component, cfl_alpha_idx, cfl_alpha_signs, alpha_q3 of every evaluation, in order */
} T;

static void hook_predict(const int16_t *q3, uint8_t *pred, int32_t pred_stride, uint8_t *dst, int32_t dst_stride, int32_t alpha_q3, int32_t bd,
                         int32_t w, int32_t h)
{
    (void)q3; (void)pred; (void)pred_stride; (void)dst; (void)dst_stride; (void)bd; (void)w; (void)h;
    T.alpha_q3 = alpha_q3;
}

static void hook_residual(uint8_t *in, uint32_t is, uint8_t *pred, uint32_t ps, int16_t *res, uint32_t rs, uint32_t w, uint32_t h)
{
    (void)in; (void)is; (void)pred; (void)ps; (void)res; (void)rs; (void)w; (void)h;
}

void FullLoop_R(LargestCodingUnit_t *sb_ptr, ModeDecisionCandidateBuffer_t *candidateBuffer, ModeDecisionContext_t *context_ptr,
                EbPictureBufferDesc_t *inputPicturePtr, PictureControlSet_t *picture_control_set_ptr, uint32_t component_mask, uint32_t cbQp,
                uint32_t crQp, uint32_t *cbCountNonZeroCoeffs, uint32_t *crCountNonZeroCoeffs)
{
    (void)sb_ptr; (void)candidateBuffer; (void)context_ptr; (void)inputPicturePtr; (void)picture_control_set_ptr; (void)component_mask;
    (void)cbQp; (void)crQp;
    *cbCountNonZeroCoeffs = 1;
    *crCountNonZeroCoeffs = 1;
}

void CuFullDistortionFastTuMode_R(LargestCodingUnit_t *sb_ptr, ModeDecisionCandidateBuffer_t *candidateBuffer, ModeDecisionContext_t *context_ptr,
                                  ModeDecisionCandidate_t *candidate_ptr, PictureControlSet_t *picture_control_set_ptr,
                                  uint64_t cbFullDistortion[DIST_CALC_TOTAL], uint64_t crFullDistortion[DIST_CALC_TOTAL],
                                  uint32_t count_non_zero_coeffs[3][MAX_NUM_OF_TU_PER_CU], COMPONENT_TYPE componentType, uint64_t *cb_coeff_bits,
                                  uint64_t *cr_coeff_bits, EbAsm asm_type)
{
    (void)sb_ptr; (void)candidateBuffer; (void)context_ptr; (void)picture_control_set_ptr; (void)count_non_zero_coeffs; (void)asm_type;
    const int plane = componentType == COMPONENT_CHROMA_CB ? 0 : 1, k = T.alpha_q3 + 16;
    if (T.n_keys < 256) {
        int32_t *key = T.keys[T.n_keys++];
        key[0] = plane; key[1] = candidate_ptr->cfl_alpha_idx; key[2] = candidate_ptr->cfl_alpha_signs; key[3] = T.alpha_q3;
    }
    T.mask[plane] |= 1ull << k;
    if (plane == 0) {
        cbFullDistortion[DIST_CALC_RESIDUAL] = T.dist[k];
        *cb_coeff_bits = T.bits[k];
    } else {
        crFullDistortion[DIST_CALC_RESIDUAL] = T.dist[33 + k];
        *cr_coeff_bits = T.bits[33 + k];
    }
}

int drv_subsample(int bit_depth, void *luma, int stride, int w, int h, int16_t *q3)
{
    if (bit_depth == 8) cfl_luma_subsampling_420_lbd_c((uint8_t *)luma, stride, q3, w, h);
    else cfl_luma_subsampling_420_hbd_c((const uint16_t *)luma, stride, q3, w, h);
    return 0;
}

int drv_subtract_average(int avx2, int16_t *q3, int cw, int ch)
{
    (avx2 ? subtract_average_avx2 : subtract_average_c)(q3, cw, ch, cw * ch / 2, __builtin_ctz(cw) + __builtin_ctz(ch));
    return 0;
}

int drv_predict(int avx2, int bit_depth, const int16_t *q3, void *pred, int pred_stride, void *dst, int dst_stride, int alpha_q3, int cw, int ch)
{
    if (bit_depth == 8)
        (avx2 ? cfl_predict_lbd_avx2 : cfl_predict_lbd_c)(q3, (uint8_t *)pred, pred_stride, (uint8_t *)dst, dst_stride, alpha_q3, 8, cw, ch);
    else
        (avx2 ? cfl_predict_hbd_avx2 : cfl_predict_hbd_c)(q3, (uint16_t *)pred, pred_stride, (uint16_t *)dst, dst_stride, alpha_q3, bit_depth, cw,
                                                         ch);
    return 0;
}

int drv_idx_to_alpha(int idx, int joint_sign, int plane) { return cfl_idx_to_alpha(idx, joint_sign, plane ? CFL_PRED_V : CFL_PRED_U); }

/* bits / dist: [2][33] by plane and alpha_q3 + 16; alpha_bits: cflAlphaFacBits[8][2][16]; out[3] = intra_chroma_mode, cfl_alpha_idx,
 * cfl_alpha_signs; masks[2]; keys[256][4] and the number of evaluations (may be NULL) */
int drv_pick_alpha(const uint64_t *bits, const uint64_t *dist, uint64_t lambda, const int32_t *alpha_bits, int cfl_mode_bits, int dc_mode_bits,
                   int cw, int ch, int32_t *out, uint64_t *masks, int32_t *keys, int32_t *n_keys)
{
    static ModeDecisionContext_t *ctx;
    static ModeDecisionCandidateBuffer_t *cb;
    static ModeDecisionCandidate_t *cand;
    static MdRateEstimationContext_t *rate;
    static EbPictureBufferDesc_t *pic[4];
    static BlockGeom geom;
    if (!ctx) {
        ctx = (ModeDecisionContext_t *)calloc(1, sizeof(*ctx));
        cb = (ModeDecisionCandidateBuffer_t *)calloc(1, sizeof(*cb));
        cand = (ModeDecisionCandidate_t *)calloc(1, sizeof(*cand));
        rate = (MdRateEstimationContext_t *)calloc(1, sizeof(*rate));
        for (int i = 0; i < 4; i++) {
            pic[i] = (EbPictureBufferDesc_t *)calloc(1, sizeof(EbPictureBufferDesc_t));
            pic[i]->bufferCb = (EbByte)calloc(1, 4096);
            pic[i]->bufferCr = (EbByte)calloc(1, 4096);
            pic[i]->strideCb = pic[i]->strideCr = 16;
        }
        cb->candidate_ptr = cand;
        cb->prediction_ptr = pic[0];
        cb->cflTempPredictionPtr = pic[1];
        cb->residual_ptr = pic[2];
        cand->md_rate_estimation_ptr = rate;
        ctx->blk_geom = &geom;
        cfl_predict_lbd = hook_predict;
        ResidualKernel = hook_residual;
    }
    geom.bwidth_uv = (uint8_t)cw;
    geom.bheight_uv = (uint8_t)ch;
    ctx->full_lambda = (uint32_t)lambda;
    if (ctx->full_lambda != lambda) return -1;
    cand->intra_luma_mode = DC_PRED;
    cand->intra_chroma_mode = UV_CFL_PRED;
    memcpy(rate->cflAlphaFacBits, alpha_bits, sizeof(rate->cflAlphaFacBits));
    if (sizeof(rate->cflAlphaFacBits) != 8 * 2 * 16 * sizeof(int32_t)) return -2;
    rate->intraUVmodeFacBits[CFL_ALLOWED][DC_PRED][UV_CFL_PRED] = cfl_mode_bits;
    rate->intraUVmodeFacBits[CFL_ALLOWED][DC_PRED][UV_DC_PRED] = dc_mode_bits;
    T.bits = bits;
    T.dist = dist;
    T.mask[0] = T.mask[1] = 0;
    T.n_keys = 0;
    cfl_rd_pick_alpha(NULL, cb, NULL, ctx, pic[3], 0, 0, ASM_NON_AVX2);
    out[0] = cand->intra_chroma_mode;
    out[1] = cand->cfl_alpha_idx;
    out[2] = cand->cfl_alpha_signs;
    masks[0] = T.mask[0];
    masks[1] = T.mask[1];
    if (keys) memcpy(keys, T.keys, sizeof(T.keys));
    if (n_keys) *n_keys = T.n_keys;
    return 0;
}
