/*
 * tests/golden/ref_ma_stats_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own motion-analysis functions for tests/golden/make_golden_ma_stats.py, tests/test_ma_stats_vs_ref.py and
 * tools/ma_stats_probe.py --cpu.  Contains no reference code: it builds the objects those functions read (a sequence control set whose SB
 * parameters come from the reference's sb_params_init, a parent picture control set with its per-SB tables, ME results and OIS results, the
 * previous picture's control set behind its wrapper, a PA reference object, pictures with 68 / 16 border samples) and calls
 *   ComputeDecimatedZzSad                                   Codec/EbMotionEstimationProcess.c:219
 *   CalculateAcEnergy, FailingMotionLcu, DetectUncoveredLcu Codec/EbSourceBasedOperationsProcess.c:347, :214, :273
 *   MeBasedGlobalMotionDetection, DeriveSimilarCollocatedFlag   Codec/EbInitialRateControlProcess.c:467, :1286
 * with asm_type = ASM_AVX2 as the encoder.
 *   drv_ma_open    a width x height geometry; returns the number of SBs
 *   drv_ma_zz      the unpadded luma of the current and the previous picture -> zz_cost, non_moving_index [n_sb] as ComputeDecimatedZzSad
 *                  stores them in the PREVIOUS picture's control set, and sad [n_sb].  ComputeDecimatedZzSad keeps the SAD in a local, so
 *                  the driver makes the same two calls it makes (Decimation2D, NxMSadKernel_funcPtrArray[asm][2]) for the SAD itself.
 *   drv_ma_energy  the unpadded luma, slice_is_intra, y_mean [n_sb][85] -> energy, mean [n_sb][5]
 *   drv_ma_tables  ME rows [n_sb][85] (the 24-byte layout of svthip_me_cu_result), OIS words [n_sb][85][18], this picture's y_mean / variance
 *                  [n_sb][85], the list-0 reference's yMean / variance [n_sb], signals[5] = slice_is_intra, temporal_layer_index,
 *                  hierarchical_levels, is_used_as_reference_flag, intensity_transition_flag
 *                  -> global_motion[6] = is_pan, is_tilt, panMvx, panMvy, tiltMvx, tiltMvy (the counters are locals of DetectGlobalMotion);
 *                     flags [n_sb][4] = similar_colocated_sb_array, similar_colocated_sb_array_ii, failing_motion_sb_flag, uncovered_area_sb_flag.
 *                  panMv / tiltMv are set to 0 before the call: the reference leaves them alone on an intra picture.  The two SB flags are
 *                  set to EB_FALSE before FailingMotionLcu / DetectUncoveredLcu, as source_based_operations_kernel does (:1062, :1072); both
 *                  functions repeat the conditions their caller tests, so they are called for every SB.
 *   drv_ma_time    seconds of `reps` runs of function group `which` (0 ZZ SAD, 1 AC energy, 2 the table functions) on the inputs of the
 *                  last call of that group (the CPU yardstick)
 * The rc_me_distortion sum and the distortion-histogram loop are inline in MotionEstimateLcu and in the ME thread's body: no call reaches them.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbDefinitions.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbReferenceObject.h"
#include "EbMotionEstimationProcess.h"
#include "EbMotionEstimationContext.h"
#include "EbComputeSAD.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

void Decimation2D(uint8_t *input_samples, uint32_t inputStride, uint32_t inputAreaWidth, uint32_t inputAreaHeight, uint8_t *decimSamples,
                  uint32_t decimStride, uint32_t decimStep);
EbErrorType ComputeDecimatedZzSad(MotionEstimationContext_t *context_ptr, SequenceControlSet_t *scs, PictureParentControlSet_t *pcs,
                                  EbPictureBufferDesc_t *sixteenth, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1);
void CalculateAcEnergy(SequenceControlSet_t *scs, PictureParentControlSet_t *pcs, uint32_t sb_index);
void FailingMotionLcu(SequenceControlSet_t *scs, PictureParentControlSet_t *pcs, uint32_t sb_index);
void DetectUncoveredLcu(SequenceControlSet_t *scs, PictureParentControlSet_t *pcs, uint32_t sb_index);
void MeBasedGlobalMotionDetection(PictureParentControlSet_t *pcs);
void DeriveSimilarCollocatedFlag(PictureParentControlSet_t *pcs);

#define PAD 68
#define PAD16 16

typedef struct {   /* svthip_me_cu_result */
    int16_t xMvL0, yMvL0, xMvL1, yMvL1;
    uint32_t distortion[3];
    uint8_t direction[3];
    uint8_t totalMeCandidateIndex;
} drv_me_row;

static struct {
    int w, h, n_sb, nx, ny;
    SequenceControlSet_t *scs;
    EncodeContext_t *enc;
    PictureParentControlSet_t *pcs, *prev;
    EbObjectWrapper_t prev_wrapper, ref_wrapper;
    EbPaReferenceObject_t *ref;
    MotionEstimationContext_t me_ctx;
    MeContext_t *me;
    EbPictureBufferDesc_t cur_full, prev_full, sixteenth;
    uint8_t *mem[3], sb16[16 * 16];
    OisCandidate_t *ois_words;
    EbMemoryMapEntry map[64];
    uint32_t map_index;
    uint64_t lib_memory;
} G;

void drv_ma_close(void)
{
    if (!G.pcs) return;
    PictureParentControlSet_t *p = G.pcs;
    for (int i = 0; i < G.n_sb; i++) {
        free(p->yMean[i]); free(p->variance[i]); free(p->sb_y_src_energy_cu_array[i]); free(p->sb_y_src_mean_cu_array[i]);
        free(p->me_results[i]); free(p->ois_cu32_cu16_results[i]);
    }
    free(p->yMean); free(p->variance); free(p->sb_y_src_energy_cu_array); free(p->sb_y_src_mean_cu_array); free(p->me_results);
    free(p->ois_cu32_cu16_results); free(p->similar_colocated_sb_array); free(p->similar_colocated_sb_array_ii);
    free(p->failing_motion_sb_flag); free(p->uncovered_area_sb_flag);
    free(G.prev->zz_cost_array); free(G.prev->non_moving_index_array);
    free(G.ois_words); free(G.ref); free(G.me); free(G.enc);
    free(G.scs->sb_params_array);
    for (int i = 0; i < 3; i++) free(G.mem[i]);
    free(G.scs); free(G.pcs); free(G.prev);
    memset(&G, 0, sizeof(G));
}

static void picture(EbPictureBufferDesc_t *d, uint8_t **mem, int w, int h, int pad)
{
    d->origin_x = d->origin_y = (uint16_t)pad;
    d->width = d->maxWidth = (uint16_t)w, d->height = d->maxHeight = (uint16_t)h;
    d->strideY = (uint16_t)(w + 2 * pad);
    *mem = (uint8_t *)calloc((size_t)d->strideY * (h + 2 * pad), 1);
    d->bufferY = *mem;
}

static void fill(EbPictureBufferDesc_t *d, const uint8_t *luma)
{
    for (int y = 0; y < d->height; y++) memcpy(d->bufferY + (size_t)(d->origin_y + y) * d->strideY + d->origin_x, luma + (size_t)y * d->width, d->width);
}

int drv_ma_open(int w, int h)
{
    drv_ma_close();
    memoryMap = G.map, memoryMapIndex = &G.map_index, totalLibMemory = &G.lib_memory;
    G.w = w, G.h = h, G.nx = (w + 63) / 64, G.ny = (h + 63) / 64, G.n_sb = G.nx * G.ny;
    G.scs = (SequenceControlSet_t *)calloc(1, sizeof(*G.scs));
    G.enc = (EncodeContext_t *)calloc(1, sizeof(*G.enc));
    G.pcs = (PictureParentControlSet_t *)calloc(1, sizeof(*G.pcs));
    G.prev = (PictureParentControlSet_t *)calloc(1, sizeof(*G.prev));
    G.ref = (EbPaReferenceObject_t *)calloc(1, sizeof(*G.ref));
    G.me = (MeContext_t *)calloc(1, sizeof(*G.me));
    SequenceControlSet_t *s = G.scs;
    PictureParentControlSet_t *p = G.pcs;
    s->sb_sz = 64;
    s->luma_width = (uint16_t)w, s->luma_height = (uint16_t)h;
    s->chroma_width = (uint16_t)(w / 2), s->chroma_height = (uint16_t)(h / 2);
    s->input_resolution = INPUT_SIZE_576p_RANGE_OR_LOWER;
    if (sb_params_init(s) != EB_ErrorNone) return -1;
    s->picture_width_in_sb = (uint8_t)G.nx;
    s->sb_total_count = p->sb_total_count = (uint16_t)G.n_sb;
    s->encode_context_ptr = G.enc;
    G.enc->asm_type = ASM_AVX2;
    G.me_ctx.me_context_ptr = G.me;
    G.me->sixteenth_sb_buffer = G.sb16, G.me->sixteenth_sb_buffer_stride = 16;

    p->yMean = (uint8_t **)calloc(G.n_sb, sizeof(void *)), p->variance = (uint16_t **)calloc(G.n_sb, sizeof(void *));
    p->sb_y_src_energy_cu_array = (uint64_t **)calloc(G.n_sb, sizeof(void *)), p->sb_y_src_mean_cu_array = (uint64_t **)calloc(G.n_sb, sizeof(void *));
    p->me_results = (MeCuResults_t **)calloc(G.n_sb, sizeof(void *));
    p->ois_cu32_cu16_results = (OisCu32Cu16Results_t **)calloc(G.n_sb, sizeof(void *));
    G.ois_words = (OisCandidate_t *)calloc((size_t)G.n_sb * 21 * 18, sizeof(OisCandidate_t));
    for (int i = 0; i < G.n_sb; i++) {
        p->yMean[i] = (uint8_t *)calloc(85, 1), p->variance[i] = (uint16_t *)calloc(85, 2);
        p->sb_y_src_energy_cu_array[i] = (uint64_t *)calloc(5, 8), p->sb_y_src_mean_cu_array[i] = (uint64_t *)calloc(5, 8);
        p->me_results[i] = (MeCuResults_t *)calloc(85, sizeof(MeCuResults_t));
        p->ois_cu32_cu16_results[i] = (OisCu32Cu16Results_t *)calloc(1, sizeof(OisCu32Cu16Results_t));
        for (int cu = 0; cu < 21; cu++) p->ois_cu32_cu16_results[i]->sorted_ois_candidate[cu] = G.ois_words + ((size_t)i * 21 + cu) * 18;
    }
    p->similar_colocated_sb_array = (EbBool *)calloc(G.n_sb, sizeof(EbBool)), p->similar_colocated_sb_array_ii = (EbBool *)calloc(G.n_sb, sizeof(EbBool));
    p->failing_motion_sb_flag = (uint8_t *)calloc(G.n_sb, 1), p->uncovered_area_sb_flag = (EbBool *)calloc(G.n_sb, sizeof(EbBool));
    G.prev->zz_cost_array = (uint8_t *)calloc(G.n_sb, 1), G.prev->non_moving_index_array = (uint8_t *)calloc(G.n_sb, 1);

    picture(&G.cur_full, &G.mem[0], w, h, PAD);
    picture(&G.prev_full, &G.mem[1], w, h, PAD);
    picture(&G.sixteenth, &G.mem[2], w >> 2, h >> 2, PAD16);
    p->enhanced_picture_ptr = &G.cur_full;
    G.prev->enhanced_picture_ptr = &G.prev_full;
    G.prev_wrapper.objectPtr = G.prev, p->previous_picture_control_set_wrapper_ptr = &G.prev_wrapper;
    G.ref_wrapper.objectPtr = G.ref, p->ref_pa_pic_ptr_array[0] = &G.ref_wrapper;
    return G.n_sb;
}

static void zz(void) { ComputeDecimatedZzSad(&G.me_ctx, G.scs, G.pcs, &G.sixteenth, 0, (uint32_t)G.nx, 0, (uint32_t)G.ny); }

int drv_ma_zz(const uint8_t *cur_luma, const uint8_t *prev_luma, uint32_t *sad, uint8_t *zz_cost, uint8_t *non_moving_index)
{
    if (!G.pcs) return -1;
    fill(&G.cur_full, cur_luma), fill(&G.prev_full, prev_luma);
    EbPictureBufferDesc_t *c = &G.cur_full, *q = &G.sixteenth, *v = &G.prev_full;
    Decimation2D(c->bufferY + (size_t)PAD * c->strideY + PAD, c->strideY, G.w, G.h, q->bufferY + (size_t)PAD16 * q->strideY + PAD16, q->strideY, 4);
    zz();
    memcpy(zz_cost, G.prev->zz_cost_array, G.n_sb), memcpy(non_moving_index, G.prev->non_moving_index_array, G.n_sb);
    for (int i = 0; i < G.n_sb; i++) {
        const SbParams_t *sp = &G.scs->sb_params_array[i];
        sad[i] = ~0u;
        if (!sp->is_complete_sb) continue;
        Decimation2D(v->bufferY + (size_t)(PAD + sp->origin_y) * v->strideY + PAD + sp->origin_x, v->strideY, 64, 64, G.sb16, 16, 4);
        sad[i] = NxMSadKernel_funcPtrArray[ASM_AVX2][2](q->bufferY + (size_t)(PAD16 + (sp->origin_y >> 2)) * q->strideY + PAD16 + (sp->origin_x >> 2),
                                                        q->strideY, G.sb16, 16, 16, 16);
    }
    return 0;
}

static void energy(void)
{
    for (int i = 0; i < G.n_sb; i++) CalculateAcEnergy(G.scs, G.pcs, (uint32_t)i);
}

int drv_ma_energy(const uint8_t *luma, int slice_is_intra, const uint8_t *y_mean, uint64_t *energy_out, uint64_t *mean_out)
{
    if (!G.pcs) return -1;
    fill(&G.cur_full, luma);
    G.pcs->slice_type = slice_is_intra ? I_SLICE : B_SLICE;
    for (int i = 0; i < G.n_sb; i++) memcpy(G.pcs->yMean[i], y_mean + 85 * i, 85);
    energy();
    for (int i = 0; i < G.n_sb; i++) memcpy(energy_out + 5 * i, G.pcs->sb_y_src_energy_cu_array[i], 40), memcpy(mean_out + 5 * i, G.pcs->sb_y_src_mean_cu_array[i], 40);
    return 0;
}

static void tables(void)
{
    PictureParentControlSet_t *p = G.pcs;
    p->panMvx = p->panMvy = p->tiltMvx = p->tiltMvy = 0;
    MeBasedGlobalMotionDetection(p);
    DeriveSimilarCollocatedFlag(p);
    for (int i = 0; i < G.n_sb; i++) {
        p->failing_motion_sb_flag[i] = EB_FALSE;
        FailingMotionLcu(G.scs, p, (uint32_t)i);
        p->uncovered_area_sb_flag[i] = EB_FALSE;
        DetectUncoveredLcu(G.scs, p, (uint32_t)i);
    }
}

int drv_ma_tables(const drv_me_row *me, const uint32_t *ois, const uint8_t *y_mean, const uint16_t *variance, const uint8_t *ref_mean,
                  const uint16_t *ref_var, const int32_t *signals, int32_t *global_motion, uint8_t *flags)
{
    PictureParentControlSet_t *p = G.pcs;
    if (!p) return -1;
    p->slice_type = signals[0] ? I_SLICE : B_SLICE;
    p->temporal_layer_index = (uint8_t)signals[1], p->hierarchical_levels = (uint8_t)signals[2];
    p->is_used_as_reference_flag = (EbBool)signals[3], p->intensity_transition_flag = (EbBool)signals[4];
    for (int i = 0; i < G.n_sb; i++) {
        for (int pu = 0; pu < 85; pu++) {
            const drv_me_row *r = me + (size_t)i * 85 + pu;
            MeCuResults_t *m = &p->me_results[i][pu];
            m->xMvL0 = r->xMvL0, m->yMvL0 = r->yMvL0, m->xMvL1 = r->xMvL1, m->yMvL1 = r->yMvL1;
            for (int k = 0; k < 3; k++) m->distortionDirection[k].distortion = r->distortion[k], m->distortionDirection[k].direction = r->direction[k];
            m->totalMeCandidateIndex = r->totalMeCandidateIndex;
        }
        for (int cu = 0; cu < 21; cu++)
            for (int k = 0; k < 18; k++) G.ois_words[((size_t)i * 21 + cu) * 18 + k].ois_results = ois[((size_t)i * 85 + cu) * 18 + k];
        memcpy(p->yMean[i], y_mean + 85 * i, 85), memcpy(p->variance[i], variance + 85 * i, 170);
        G.ref->yMean[i] = ref_mean[i], G.ref->variance[i] = ref_var[i];
    }
    tables();
    global_motion[0] = p->is_pan, global_motion[1] = p->is_tilt;
    global_motion[2] = p->panMvx, global_motion[3] = p->panMvy, global_motion[4] = p->tiltMvx, global_motion[5] = p->tiltMvy;
    for (int i = 0; i < G.n_sb; i++) {
        flags[4 * i + 0] = (uint8_t)p->similar_colocated_sb_array[i], flags[4 * i + 1] = (uint8_t)p->similar_colocated_sb_array_ii[i];
        flags[4 * i + 2] = (uint8_t)p->failing_motion_sb_flag[i], flags[4 * i + 3] = (uint8_t)p->uncovered_area_sb_flag[i];
    }
    return 0;
}

double drv_ma_time(int which, int reps)
{
    struct timespec a, b;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int i = 0; i < reps; i++) {
        if (which == 0) zz(); else if (which == 1) energy(); else tables();
    }
    clock_gettime(CLOCK_MONOTONIC, &b);
    return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec);
}
