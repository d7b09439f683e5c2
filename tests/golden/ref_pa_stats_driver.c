/*
 * tests/golden/ref_pa_stats_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own GatheringPictureStatistics (Codec/EbPictureAnalysisProcess.c:4742-4796) for
 * tests/golden/make_golden_pa_stats.py, tests/test_pa_stats_vs_ref.py and tools/pa_stats_probe.py --cpu.  Contains no reference code:
 * it builds the objects that function reads (a sequence control set whose SB parameters come from the reference's sb_params_init, a
 * parent picture control set with its per-SB tables and histogram arrays, the input picture with 68 luma / 34 chroma border samples,
 * the padded luma plane from the reference's generate_padding, the 1/16 plane from its Decimation2D and generate_padding) and calls
 * it with scd_mode = SCD_MODE_1 and asm_type = ASM_AVX2 as the encoder, in either block_mean_calc_prec.
 *   drv_pa_stats_open    the three unpadded planes of a width x height picture; returns the number of SBs
 *   drv_pa_stats_run     GatheringPictureStatistics at one precision; copies out
 *                        y_mean, variance [n_sb][85]; cb_mean, cr_mean [n_sb][21]; var_of_var [n_sb][4]; homogeneous [n_sb];
 *                        picture[4] = pic_avg_variance, very_low_var_pic_flag, logo_pic_flag, complete SBs;
 *                        histogram [4][4][3][256]; region_intensity [4][4][3]; average_intensity [3]
 *   drv_pa_stats_time    seconds of `reps` calls of GatheringPictureStatistics on the open picture (the CPU yardstick)
 * picture_number is 1, so EdgeDetectionMeanLumaChroma16x16 (every 4th picture) only returns; EdgeDetection runs on tables of its own.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbDefinitions.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbMcp.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

void Decimation2D(uint8_t *input_samples, uint32_t inputStride, uint32_t inputAreaWidth, uint32_t inputAreaHeight, uint8_t *decimSamples,
                  uint32_t decimStride, uint32_t decimStep);
void GatheringPictureStatistics(SequenceControlSet_t *scs, PictureParentControlSet_t *pcs, EbPictureBufferDesc_t *input,
                                EbPictureBufferDesc_t *input_padded, EbPictureBufferDesc_t *sixteenth, uint32_t sb_total_count, EbAsm asm_type);

#define PAD 68
#define PAD16 16
#define REGIONS 4

static struct {
    int w, h, n_sb, complete;
    SequenceControlSet_t *scs;
    PictureParentControlSet_t *pcs;
    EbPictureBufferDesc_t input, sixteenth;
    uint8_t *mem[4];
    EbMemoryMapEntry map[64];
    uint32_t map_index;
    uint64_t lib_memory;
} G;

void drv_pa_stats_close(void)
{
    if (!G.pcs) return;
    PictureParentControlSet_t *p = G.pcs;
    for (int i = 0; i < G.n_sb; i++) {
        free(p->yMean[i]); free(p->cbMean[i]); free(p->crMean[i]); free(p->variance[i]); free(p->var_of_var32x32_based_sb_array[i]);
    }
    for (int x = 0; x < REGIONS; x++) {
        for (int y = 0; y < REGIONS; y++) {
            for (int c = 0; c < 3; c++) free(p->picture_histogram[x][y][c]);
            free(p->picture_histogram[x][y]);
        }
        free(p->picture_histogram[x]);
    }
    free(p->picture_histogram);
    free(p->yMean); free(p->cbMean); free(p->crMean); free(p->variance); free(p->var_of_var32x32_based_sb_array);
    free(p->sb_homogeneous_area_array); free(p->edge_results_ptr); free(p->sharp_edge_sb_flag); free(p->sb_stat_array);
    free(G.scs->sb_params_array);
    for (int i = 0; i < 4; i++) free(G.mem[i]);
    free(G.scs); free(G.pcs);
    memset(&G, 0, sizeof(G));
}

int drv_pa_stats_open(int w, int h, const uint8_t *luma, const uint8_t *cb, const uint8_t *cr)
{
    drv_pa_stats_close();
    memoryMap = G.map, memoryMapIndex = &G.map_index, totalLibMemory = &G.lib_memory;
    G.w = w, G.h = h;
    G.scs = (SequenceControlSet_t *)calloc(1, sizeof(*G.scs));
    G.pcs = (PictureParentControlSet_t *)calloc(1, sizeof(*G.pcs));
    SequenceControlSet_t *s = G.scs;
    PictureParentControlSet_t *p = G.pcs;
    s->sb_sz = 64;
    s->luma_width = (uint16_t)w, s->luma_height = (uint16_t)h;
    s->chroma_width = (uint16_t)(w / 2), s->chroma_height = (uint16_t)(h / 2);
    s->picture_analysis_number_of_regions_per_width = s->picture_analysis_number_of_regions_per_height = REGIONS;
    s->scd_mode = SCD_MODE_1;
    s->input_resolution = INPUT_SIZE_576p_RANGE_OR_LOWER;
    if (sb_params_init(s) != EB_ErrorNone) return -1;
    G.n_sb = ((w + 63) / 64) * ((h + 63) / 64);
    s->sb_total_count = p->sb_total_count = (uint16_t)G.n_sb;
    for (int i = 0; i < G.n_sb; i++) G.complete += s->sb_params_array[i].is_complete_sb;
    p->picture_number = 1;
    p->yMean = (uint8_t **)calloc(G.n_sb, sizeof(void *)), p->cbMean = (uint8_t **)calloc(G.n_sb, sizeof(void *));
    p->crMean = (uint8_t **)calloc(G.n_sb, sizeof(void *)), p->variance = (uint16_t **)calloc(G.n_sb, sizeof(void *));
    p->var_of_var32x32_based_sb_array = (uint64_t **)calloc(G.n_sb, sizeof(void *));
    for (int i = 0; i < G.n_sb; i++) {
        p->yMean[i] = (uint8_t *)calloc(85, 1), p->variance[i] = (uint16_t *)calloc(85, 2);
        p->cbMean[i] = (uint8_t *)calloc(21, 1), p->crMean[i] = (uint8_t *)calloc(21, 1);
        p->var_of_var32x32_based_sb_array[i] = (uint64_t *)calloc(4, 8);
    }
    p->sb_homogeneous_area_array = (EbBool *)calloc(G.n_sb, sizeof(EbBool));
    p->edge_results_ptr = (EdgeLcuResults_t *)calloc(G.n_sb, sizeof(EdgeLcuResults_t));
    p->sharp_edge_sb_flag = (uint8_t *)calloc(G.n_sb, 1);
    p->sb_stat_array = (SbStat_t *)calloc(G.n_sb, sizeof(SbStat_t));
    p->picture_histogram = (uint32_t ****)calloc(REGIONS, sizeof(void *));
    for (int x = 0; x < REGIONS; x++) {
        p->picture_histogram[x] = (uint32_t ***)calloc(REGIONS, sizeof(void *));
        for (int y = 0; y < REGIONS; y++) {
            p->picture_histogram[x][y] = (uint32_t **)calloc(3, sizeof(void *));
            for (int c = 0; c < 3; c++) p->picture_histogram[x][y][c] = (uint32_t *)calloc(HISTOGRAM_NUMBER_OF_BINS, 4);
        }
    }
    /* the input picture: luma with a 68-sample border filled by generate_padding (it serves as the padded picture too), chroma with 34 */
    EbPictureBufferDesc_t *d = &G.input;
    d->origin_x = d->origin_y = PAD;
    d->width = d->maxWidth = (uint16_t)w, d->height = d->maxHeight = (uint16_t)h;
    d->strideY = (uint16_t)(w + 2 * PAD), d->strideCb = d->strideCr = (uint16_t)(w / 2 + PAD);
    G.mem[0] = (uint8_t *)calloc((size_t)d->strideY * (h + 2 * PAD), 1);
    G.mem[1] = (uint8_t *)calloc((size_t)d->strideCb * (h / 2 + PAD), 1);
    G.mem[2] = (uint8_t *)calloc((size_t)d->strideCr * (h / 2 + PAD), 1);
    d->bufferY = G.mem[0], d->bufferCb = G.mem[1], d->bufferCr = G.mem[2];
    for (int y = 0; y < h; y++) memcpy(d->bufferY + (size_t)(PAD + y) * d->strideY + PAD, luma + (size_t)y * w, w);
    for (int y = 0; y < h / 2; y++) {
        memcpy(d->bufferCb + (size_t)(PAD / 2 + y) * d->strideCb + PAD / 2, cb + (size_t)y * (w / 2), w / 2);
        memcpy(d->bufferCr + (size_t)(PAD / 2 + y) * d->strideCr + PAD / 2, cr + (size_t)y * (w / 2), w / 2);
    }
    generate_padding(d->bufferY, d->strideY, w, h, PAD, PAD);
    EbPictureBufferDesc_t *q = &G.sixteenth;
    q->origin_x = q->origin_y = PAD16;
    q->width = q->maxWidth = (uint16_t)(w >> 2), q->height = q->maxHeight = (uint16_t)(h >> 2);
    q->strideY = (uint16_t)((w >> 2) + 2 * PAD16);
    G.mem[3] = (uint8_t *)calloc((size_t)q->strideY * ((h >> 2) + 2 * PAD16), 1);
    q->bufferY = G.mem[3];
    Decimation2D(d->bufferY + (size_t)PAD * d->strideY + PAD, d->strideY, w, h, q->bufferY + (size_t)PAD16 * q->strideY + PAD16, q->strideY, 4);
    generate_padding(q->bufferY, q->strideY, w >> 2, h >> 2, PAD16, PAD16);
    return G.n_sb;
}

static void gather(int sub_precision)
{
    G.scs->block_mean_calc_prec = sub_precision ? BLOCK_MEAN_PREC_SUB : BLOCK_MEAN_PREC_FULL;
    GatheringPictureStatistics(G.scs, G.pcs, &G.input, &G.input, &G.sixteenth, (uint32_t)G.n_sb, ASM_AVX2);
}

int drv_pa_stats_run(int sub_precision, uint8_t *y_mean, uint16_t *variance, uint8_t *cb_mean, uint8_t *cr_mean, uint64_t *var_of_var,
                     uint8_t *homogeneous, uint32_t *picture, uint32_t *histogram, uint32_t *region_intensity, uint32_t *average_intensity)
{
    PictureParentControlSet_t *p = G.pcs;
    if (!p) return -1;
    gather(sub_precision);
    for (int i = 0; i < G.n_sb; i++) {
        memcpy(y_mean + 85 * i, p->yMean[i], 85), memcpy(variance + 85 * i, p->variance[i], 170);
        memcpy(cb_mean + 21 * i, p->cbMean[i], 21), memcpy(cr_mean + 21 * i, p->crMean[i], 21);
        memcpy(var_of_var + 4 * i, p->var_of_var32x32_based_sb_array[i], 32);
        homogeneous[i] = (uint8_t)p->sb_homogeneous_area_array[i];
    }
    picture[0] = p->pic_avg_variance, picture[1] = p->very_low_var_pic_flag, picture[2] = p->logo_pic_flag, picture[3] = (uint32_t)G.complete;
    for (int x = 0; x < REGIONS; x++)
        for (int y = 0; y < REGIONS; y++)
            for (int c = 0; c < 3; c++) {
                memcpy(histogram + ((x * REGIONS + y) * 3 + c) * 256, p->picture_histogram[x][y][c], 1024);
                region_intensity[(x * REGIONS + y) * 3 + c] = (uint32_t)p->average_intensity_per_region[x][y][c];
            }
    for (int c = 0; c < 3; c++) average_intensity[c] = p->average_intensity[c];
    return 0;
}

double drv_pa_stats_time(int sub_precision, int reps)
{
    struct timespec a, b;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int i = 0; i < reps; i++) gather(sub_precision);
    clock_gettime(CLOCK_MONOTONIC, &b);
    return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec);
}
