/*
 * tests/golden/ref_md_part_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Runs the reference's own partition decision on given block costs for tests/golden/make_golden_md_part.py and
 * tests/test_md_part_vs_ref.py, with stand-in structs: zeroed allocations of the reference's own types in which only the fields its
 * functions read are set.  Contains no reference code, only calls into it:
 *   drv_md_part_geometry   build_blk_geom(use_128) and the fields of blk_geom_mds (Codec/EbUtility.c:702-837) the tests compare
 *   drv_md_part_run        Initialize_cu_data_structure (Codec/EbProductCodingLoop.c:663-697), then the loop of mode_decision_sb
 *                          (:2762-2880) replayed over a leaf list with md_encode_block replaced by "the cost of this leaf is given":
 *                          per leaf the assignments of :2780-2789, d1_non_square_block_decision (Codec/EbFullLoop.c:2086-2108) when
 *                          nsi + 1 == totns, d2_inter_depth_block_decision (:2368-2437) when the d1 blocks are complete; then the walk
 *                          of EncodePass (Codec/EbCodingLoop.c:3051-3069, :4111-4114) with the reference's own offset tables.
 *                          Before the loop every cost is MAX_MODE_COST: a block no leaf names counts as that.
 *                          Before each call of d2 the driver follows the climb that call is about to make and counts, from the geometry
 *                          and the picture size alone, which arm of Av1SplitFlagRate (Codec/EbRateDistortionCost.c:2333-2373) each of its
 *                          calls takes: counters[1] calls in all, [2] with hasRows && hasCols, [3] below 8x8 (no context either).
 */
#define RTCD_C
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "EbDefinitions.h"
#include "aom_dsp_rtcd.h"
#include "EbCodingUnit.h"
#include "EbFullLoop.h"
#include "EbMdRateEstimation.h"
#include "EbModeDecisionConfigurationProcess.h"
#include "EbModeDecisionProcess.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbUtility.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

void Initialize_cu_data_structure(ModeDecisionContext_t *context_ptr, SequenceControlSet_t *sequence_control_set_ptr, LargestCodingUnit_t *sb_ptr,
                                  const MdcLcuData_t *const mdcResultTbPtr);

/* build_blk_geom takes the logarithms of the block sides with LOG2F, NASM code the link does not have: a compiler builtin stands in, as
 * in tests/golden/ref_cfl_driver.c */
uint32_t Log2f_SSE2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x | 1u); }

static struct {
    int built; /* 0 none, 1 for 64x64, 2 for 128x128 */
    ModeDecisionContext_t *ctx;
    MdRateEstimationContext_t *md;
    SequenceControlSet_t *scs;
    PictureControlSet_t *pcs;
    EbObjectWrapper_t *wrap;
    LargestCodingUnit_t *sb;
    MdcLcuData_t *mdc;
} G;

static uint32_t geometry(int use_128)
{
    if (G.built != 1 + !!use_128) {
        build_blk_geom(use_128);
        G.built = 1 + !!use_128;
    }
    return use_128 ? 4421u : 1101u;
}

#define GEOM_FIELDS 13
int drv_md_part_geometry(int use_128, int32_t *out)
{
    const uint32_t n = geometry(use_128);
    for (uint32_t i = 0; i < n; i++) {
        const BlockGeom *g = Get_blk_geom_mds(i);
        int32_t *o = out + (size_t)i * GEOM_FIELDS;
        o[0] = g->origin_x, o[1] = g->origin_y, o[2] = g->bwidth, o[3] = g->bheight, o[4] = (int32_t)g->shape, o[5] = g->depth, o[6] = g->nsi, o[7] = g->totns;
        o[8] = g->sqi_mds, o[9] = g->is_last_quadrant, o[10] = g->has_uv, o[11] = g->bwidth_uv, o[12] = g->bheight_uv;
    }
    return (int)n;
}

/* which arm Av1SplitFlagRate takes for square `mds`: recomputed from the geometry, as :2330-2337 do */
static void count_arm(uint32_t mds, uint32_t *counters)
{
    const BlockGeom *g = Get_blk_geom_mds(mds);
    counters[1]++;
    if (g->bsize < BLOCK_8X8) {
        counters[3]++;
        return;
    }
    const uint32_t hbs = g->bwidth >> 1;
    if (G.ctx->sb_origin_y + g->origin_y + hbs < G.scs->luma_height && G.ctx->sb_origin_x + g->origin_x + hbs < G.scs->luma_width) counters[2]++;
}

/* the calls of Av1SplitFlagRate that d2_inter_depth_block_decision(blk_mds) is about to make */
static void count_climb(uint32_t blk_mds, int use_128, int intra, uint32_t *counters)
{
    if (G.ctx->md_cu_arr_nsq[blk_mds].split_flag != EB_FALSE) return;
    const BlockGeom *g = Get_blk_geom_mds(blk_mds);
    uint32_t cur = blk_mds;
    while (g->is_last_quadrant) {
        const uint32_t parent = cur - parent_depth_offset[use_128][g->depth], step = ns_depth_offset[use_128][g->depth];
        if (!(intra && parent == 0)) {
            if (G.ctx->md_local_cu_unit[parent].tested_cu_flag == EB_TRUE) count_arm(parent, counters);
            count_arm(parent, counters);
            if (G.ctx->blk_geom->bsize > BLOCK_4X4)
                for (uint32_t k = 0; k < 4; k++)
                    if (G.ctx->md_cu_arr_nsq[cur - k * step].mdc_split_flag == 0) count_arm(cur - k * step, counters);
        }
        cur = parent, g = Get_blk_geom_mds(parent);
    }
}

/* leaf: [n_leaf][3] = mds_idx, tot_d1_blocks, split_flag; cost: [n_leaf].  out_cost [n_blocks]; out_state [n_blocks][5] = part, split_flag,
 * best_d1_blk, tested_cu_flag, mdc_split_flag; out_final [up to 1024] the md-scan indices EncodePass visits; counters[0] their count.
 * Returns the block count. */
int drv_md_part_run(int use_128, int intra, uint32_t luma_width, uint32_t luma_height, uint32_t sb_origin_x, uint32_t sb_origin_y, uint32_t full_lambda,
                    const int32_t *fac_bits, int n_leaf, const uint32_t *leaf, const uint64_t *cost, uint64_t *out_cost, uint32_t *out_state,
                    uint32_t *out_final, uint32_t *counters)
{
    const uint32_t n = geometry(use_128);
    if (!G.ctx) {
        G.ctx = (ModeDecisionContext_t *)calloc(1, sizeof(*G.ctx));
        G.md = (MdRateEstimationContext_t *)calloc(1, sizeof(*G.md));
        G.scs = (SequenceControlSet_t *)calloc(1, sizeof(*G.scs));
        G.pcs = (PictureControlSet_t *)calloc(1, sizeof(*G.pcs));
        G.wrap = (EbObjectWrapper_t *)calloc(1, sizeof(*G.wrap));
        G.sb = (LargestCodingUnit_t *)calloc(1, sizeof(*G.sb));
        G.mdc = (MdcLcuData_t *)calloc(1, sizeof(*G.mdc));
    }
    memset(G.ctx->md_local_cu_unit, 0, sizeof(G.ctx->md_local_cu_unit));
    memset(G.ctx->md_cu_arr_nsq, 0, sizeof(G.ctx->md_cu_arr_nsq));
    memcpy(G.md->partitionFacBits, fac_bits, sizeof(G.md->partitionFacBits));
    G.scs->sb_size = use_128 ? BLOCK_128X128 : BLOCK_64X64;
    G.scs->max_block_cnt = (uint16_t)n;
    G.scs->luma_width = (uint16_t)luma_width, G.scs->luma_height = (uint16_t)luma_height;
    G.wrap->objectPtr = G.scs;
    G.pcs->sequence_control_set_wrapper_ptr = G.wrap;
    G.pcs->slice_type = intra ? I_SLICE : P_SLICE;
    G.ctx->md_rate_estimation_ptr = G.md;
    G.ctx->full_lambda = full_lambda;
    G.ctx->sb_origin_x = sb_origin_x, G.ctx->sb_origin_y = sb_origin_y;
    memset(counters, 0, 4 * sizeof(*counters));

    Initialize_cu_data_structure(G.ctx, G.scs, G.sb, G.mdc);
    for (uint32_t i = 0; i < n; i++) G.ctx->md_local_cu_unit[i].cost = MAX_MODE_COST;

    uint32_t d1_blocks_accumlated = 0;
    for (int i = 0; i < n_leaf; i++) {
        const uint32_t blk_idx_mds = leaf[3 * i], tot_d1_blocks = leaf[3 * i + 1], split_flag = leaf[3 * i + 2];
        const BlockGeom *blk_geom = G.ctx->blk_geom = Get_blk_geom_mds(blk_idx_mds);
        CodingUnit_t *cu_ptr = G.ctx->cu_ptr = &G.ctx->md_cu_arr_nsq[blk_idx_mds];
        G.ctx->md_local_cu_unit[blk_idx_mds].tested_cu_flag = EB_TRUE;
        cu_ptr->mds_idx = (uint16_t)blk_idx_mds;
        G.ctx->md_cu_arr_nsq[blk_idx_mds].mdc_split_flag = (uint16_t)split_flag;
        cu_ptr->split_flag = (uint16_t)split_flag;
        cu_ptr->best_d1_blk = (uint16_t)blk_idx_mds;
        G.ctx->md_local_cu_unit[blk_idx_mds].cost = cost[i]; /* md_encode_block */
        if (blk_geom->nsi + 1 == blk_geom->totns) d1_non_square_block_decision(G.ctx);
        d1_blocks_accumlated = blk_geom->shape == PART_N ? 1 : d1_blocks_accumlated + 1;
        if (d1_blocks_accumlated == tot_d1_blocks) {
            count_climb(blk_geom->sqi_mds, use_128, intra, counters);
            d2_inter_depth_block_decision(G.ctx, blk_geom->sqi_mds, G.sb, 0, sb_origin_x, sb_origin_y, G.ctx->full_lambda, G.ctx->md_rate_estimation_ptr,
                                          G.pcs);
        }
    }

    for (uint32_t i = 0; i < n; i++) {
        out_cost[i] = G.ctx->md_local_cu_unit[i].cost;
        uint32_t *o = out_state + 5 * (size_t)i;
        o[0] = G.ctx->md_cu_arr_nsq[i].part, o[1] = G.ctx->md_cu_arr_nsq[i].split_flag, o[2] = G.ctx->md_cu_arr_nsq[i].best_d1_blk;
        o[3] = G.ctx->md_local_cu_unit[i].tested_cu_flag, o[4] = G.ctx->md_cu_arr_nsq[i].mdc_split_flag;
    }

    /* EncodePass's walk */
    uint32_t final_cu_itr = 0, blk_it = 0;
    while (blk_it < G.scs->max_block_cnt) {
        const PartitionType part = G.ctx->md_cu_arr_nsq[blk_it].part;
        const BlockGeom *blk_geom = Get_blk_geom_mds(blk_it);
        if (part != PARTITION_SPLIT) {
            const int32_t offset_d1 = (int32_t)ns_blk_offset[(int32_t)part], num_d1_block = (int32_t)ns_blk_num[(int32_t)part];
            for (int32_t d1_itr = (int32_t)blk_it + offset_d1; d1_itr < (int32_t)blk_it + offset_d1 + num_d1_block; d1_itr++) {
                blk_geom = Get_blk_geom_mds((uint32_t)d1_itr);
                out_final[final_cu_itr++] = (uint32_t)d1_itr;
            }
            blk_it += ns_depth_offset[use_128][blk_geom->depth];
        } else {
            blk_it += d1_depth_offset[use_128][blk_geom->depth];
        }
    }
    counters[0] = final_cu_itr;
    return (int)n;
}
