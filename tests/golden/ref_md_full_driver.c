/*
 * tests/golden/ref_md_full_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the leaves of the reference's full loop on numbers the caller gives, with stand-in structs (zeroed allocations of the reference's
 * own types in which only the fields those functions read are set), for tests/golden/make_golden_md_full.py and
 * tests/test_md_full_vs_ref.py.  Contains no reference code:
 *   drv_md_full_tu_cost_luma   Av1TuCalcCostLuma (Codec/EbRateDistortionCost.c:2152-2230)
 *   drv_md_full_tu_cost        Av1TuCalcCost (:2051-2145) with COMPONENT_CHROMA, as CuFullDistortionFastTuMode_R calls it
 *   drv_md_full_cost           Av1IntraFullCost / Av1InterFullCost (:1737-1840) -> Av1FullCost / Av1MergeSkipFullCost
 *   drv_md_full_decision       product_full_mode_decision (Codec/EbModeDecision.c:1968-2255), whole, on fabricated candidate buffers
 * AV1PerformFullLoop itself is NOT run here: the chain of transform, quantisation and rate around these leaves is pinned by the tests
 * of those entries, and the composition is restated in tests/md_full_util.py.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "EbDefinitions.h"
#include "EbCodingUnit.h"
#include "EbMdRateEstimation.h"
#include "EbModeDecision.h"
#include "EbModeDecisionProcess.h"
#include "EbRateDistortionCost.h"
#include "EbUtility.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

/* every txb_skip_cost[ctx][1] of the luma tables = zero_flag_bits: the one table entry Av1TuCalcCostLuma / Av1TuCalcCost read */
static MdRateEstimationContext_t *rate_tables(int32_t zero_flag_bits, int32_t skip_mode_bits)
{
    MdRateEstimationContext_t *t = (MdRateEstimationContext_t *)calloc(1, sizeof(*t));
    for (int s = 0; s < TX_SIZES; s++)
        for (int c = 0; c < TXB_SKIP_CONTEXTS; c++) t->coeffFacBits[s][0].txb_skip_cost[c][1] = zero_flag_bits;
    for (int c = 0; c < SKIP_CONTEXTS; c++) t->skipModeFacBits[c][1] = skip_mode_bits;
    return t;
}

/* io: dist[2], bits; out: full_cost, y_has_coeff */
int drv_md_full_tu_cost_luma(int txb_skip_ctx, int tx_size, uint32_t count_non_zero, uint64_t *dist, uint64_t *bits, uint64_t lambda,
                             int32_t zero_flag_bits, uint64_t *full_cost, uint32_t *y_has_coeff)
{
    ModeDecisionCandidate_t *cand = (ModeDecisionCandidate_t *)calloc(1, sizeof(*cand));
    cand->md_rate_estimation_ptr = rate_tables(zero_flag_bits, 0);
    cand->type = INTER_MODE;
    const EbErrorType rc = Av1TuCalcCostLuma((int16_t)txb_skip_ctx, cand, 0, (TxSize)tx_size, count_non_zero, dist, bits, full_cost, lambda);
    *y_has_coeff = cand->y_has_coeff;
    free(cand->md_rate_estimation_ptr);
    free(cand);
    return rc == EB_ErrorNone ? 0 : -1;
}

/* out: has_coeff[3] = y, u, v as COMPONENT_CHROMA leaves them (y untouched: 0) */
int drv_md_full_tu_cost(int txb_skip_ctx, int tx_size, const uint32_t *count_non_zero, uint64_t *y_dist, uint64_t *cb_dist, uint64_t *cr_dist,
                        uint64_t *bits, uint64_t lambda, uint32_t *has_coeff)
{
    ModeDecisionCandidate_t *cand = (ModeDecisionCandidate_t *)calloc(1, sizeof(*cand));
    cand->md_rate_estimation_ptr = rate_tables(0, 0);
    const EbErrorType rc = Av1TuCalcCost(cand, (int16_t)txb_skip_ctx, 0, count_non_zero[0], count_non_zero[1], count_non_zero[2], y_dist, cb_dist, cr_dist,
                                         COMPONENT_CHROMA, &bits[0], &bits[1], &bits[2], (TxSize)tx_size, lambda);
    has_coeff[0] = cand->y_has_coeff, has_coeff[1] = cand->u_has_coeff, has_coeff[2] = cand->v_has_coeff;
    free(cand->md_rate_estimation_ptr);
    free(cand);
    return rc == EB_ErrorNone ? 0 : -1;
}

/* out[6]: full cost, merge cost, skip cost, full_lambda_rate, full_cost_luma, skip_flag.  The costs start as 0 and the buffer's other
 * fields as 0, so what a function does not assign reads 0. */
int drv_md_full_cost(int is_inter, int merge_flag, int has_uv, uint64_t luma_rate, uint64_t chroma_rate, int skip_flag_context, int32_t skip_mode_bits,
                     uint64_t *y_dist, uint64_t *cb_dist, uint64_t *cr_dist, uint64_t lambda, uint64_t *bits, uint64_t *out)
{
    ModeDecisionContext_t *ctx = (ModeDecisionContext_t *)calloc(1, sizeof(*ctx));
    ModeDecisionCandidateBuffer_t *buf = (ModeDecisionCandidateBuffer_t *)calloc(1, sizeof(*buf));
    ModeDecisionCandidate_t *cand = (ModeDecisionCandidate_t *)calloc(1, sizeof(*cand));
    CodingUnit_t *cu = (CodingUnit_t *)calloc(1, sizeof(*cu));
    BlockGeom geom;
    memset(&geom, 0, sizeof(geom));
    geom.has_uv = has_uv, geom.bwidth = 16, geom.bheight = 16, geom.txb_count = 1;
    ctx->blk_geom = &geom;
    cu->skip_flag_context = (unsigned)skip_flag_context;
    cand->md_rate_estimation_ptr = rate_tables(0, skip_mode_bits);
    cand->type = is_inter ? INTER_MODE : INTRA_MODE;
    cand->merge_flag = merge_flag ? EB_TRUE : EB_FALSE;
    cand->fast_luma_rate = luma_rate, cand->fast_chroma_rate = chroma_rate;
    cand->intra_chroma_mode = UV_DC_PRED;
    uint64_t cost = 0, merge = 0, skip = 0;
    buf->candidate_ptr = cand;
    buf->full_cost_ptr = &cost, buf->full_cost_merge_ptr = &merge, buf->full_cost_skip_ptr = &skip;
    const EbErrorType rc = is_inter ? Av1InterFullCost(NULL, ctx, buf, cu, y_dist, cb_dist, cr_dist, lambda, &bits[0], &bits[1], &bits[2], BLOCK_16X16)
                                    : Av1IntraFullCost(NULL, ctx, buf, cu, y_dist, cb_dist, cr_dist, lambda, &bits[0], &bits[1], &bits[2], BLOCK_16X16);
    out[0] = cost, out[1] = merge, out[2] = skip, out[3] = buf->full_lambda_rate, out[4] = buf->full_cost_luma, out[5] = cand->skip_flag;
    free(cand->md_rate_estimation_ptr);
    free(cand), free(buf), free(cu), free(ctx);
    return rc == EB_ErrorNone ? 0 : -1;
}

/* n buffers with cost[b], type[b] (1 INTER_MODE, 2 INTRA_MODE) and pred_mode[b]; best[]: the best_candidate_index_array of `count` entries.
 * Returns lowestCostIndex; *best_intra_mode starts as 0xff; *cost = md_local_cu_unit[0].cost. */
int drv_md_full_decision(int n, const uint64_t *cost, const uint8_t *type, const uint8_t *pred_mode, const uint8_t *best, uint32_t count,
                         uint32_t *best_intra_mode, uint64_t *out_cost)
{
    if (n < 1 || n > 16 || count < 1 || count > 16) return -1;
    ModeDecisionContext_t *ctx = (ModeDecisionContext_t *)calloc(1, sizeof(*ctx));
    CodingUnit_t *cu = (CodingUnit_t *)calloc(1, sizeof(*cu));
    ModeDecisionCandidateBuffer_t *buffers = (ModeDecisionCandidateBuffer_t *)calloc((size_t)n, sizeof(*buffers));
    ModeDecisionCandidate_t *cands = (ModeDecisionCandidate_t *)calloc((size_t)n, sizeof(*cands));
    ModeDecisionCandidateBuffer_t *ptrs[16];
    uint64_t costs[16], merge[16], skip[16];
    uint8_t order[16];
    BlockGeom geom;
    memset(&geom, 0, sizeof(geom));
    geom.has_uv = 1, geom.txb_count = 1;
    ctx->blk_geom = &geom;
    ctx->cu_ptr = cu;
    for (int i = 0; i < n; i++) {
        costs[i] = cost[i], merge[i] = skip[i] = 0;
        cands[i].type = type[i];
        cands[i].pred_mode = (PredictionMode)pred_mode[i];
        buffers[i].candidate_ptr = &cands[i];
        buffers[i].full_cost_ptr = &costs[i], buffers[i].full_cost_merge_ptr = &merge[i], buffers[i].full_cost_skip_ptr = &skip[i];
        ptrs[i] = &buffers[i];
    }
    for (uint32_t i = 0; i < count; i++) {
        if (best[i] >= n) return -1;
        order[i] = best[i];
    }
    *best_intra_mode = 0xff;
    const int winner = product_full_mode_decision(ctx, cu, 16, 16, ptrs, count, order, best_intra_mode);
    *out_cost = ctx->md_local_cu_unit[0].cost;
    free(cands), free(buffers), free(cu), free(ctx);
    return winner;
}
