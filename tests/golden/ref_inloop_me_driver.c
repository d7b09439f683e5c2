/*
 * tests/golden/ref_inloop_me_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own in_loop_motion_estimation_sblock (Codec/EbProductCodingLoop.c:6300-6733) for
 * tests/golden/make_golden_inloop_me.py, tests/test_me_inloop_vs_ref.py and tools/inloop_me_probe.py.  Contains no reference code: it
 * builds an SsMeContext_t with in_loop_me_context_ctor and the minimum of a picture control set that the function reads -- the sequence
 * set with luma_width, luma_height, sb_size = BLOCK_64X64, 8-bit depth and asm_type = ASM_NON_AVX2; slice_type; ref_pic_ptr_array[list]
 * with a padded referencePicture; parent_pcs_ptr->use_subpel_flag -- and stages sb_buffer as EncDecKernel does
 * (Codec/EbEncDecProcess.c:1509-1524).
 *   drv_inloop_open   the source picture [h][w] and two reference pictures already padded by `pad` samples each way
 *                     ([h + 2 pad][w + 2 pad]); ref1 may be NULL (P slice: one list).  pad must be at least 65: the function forms the
 *                     index of the sample 2 left of and above the window in a uint32_t (:6451-6453), which wraps for a window that starts
 *                     63 samples outside the picture unless the border is that wide (the encoder's is 160)
 *   drv_inloop_run    one superblock: centres (x, y) per list, the requested area, use_subpel_flag; before the call p_sb_best_sad,
 *                     p_sb_best_mv, inloop_me_mv, the three interpolated buffers of both lists and avctemp_buffer are filled with the byte
 *                     `prefill`, so whatever the function computes from bytes it never wrote shows as a difference between two runs.  Copies out x/y_search_area_origin per list, and per list the 849 entries of
 *                     p_sb_best_sad, p_sb_best_mv and inloop_me_mv
 *   drv_inloop_time   seconds of `reps` passes over every superblock of the picture, list 0, centre (0, 0) (the CPU yardstick)
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbDefinitions.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbReferenceObject.h"
#include "EbMotionEstimationContext.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

EbErrorType in_loop_me_context_ctor(SsMeContext_t **object_dbl_ptr);
EbErrorType in_loop_motion_estimation_sblock(PictureControlSet_t *picture_control_set_ptr, uint32_t sb_origin_x, uint32_t sb_origin_y, int16_t xMvL0,
                                             int16_t yMvL0, int16_t xMvL1, int16_t yMvL1, SsMeContext_t *context_ptr);

#define N_BLOCKS 849

static struct {
    int w, h, pad, lists;
    uint8_t *src;
    SsMeContext_t *me;
    SequenceControlSet_t *scs;
    EncodeContext_t *enc;
    PictureControlSet_t *pcs;
    PictureParentControlSet_t *ppcs;
    EbObjectWrapper_t scs_wrapper, ref_wrapper[2];
    EbReferenceObject_t ref_object[2];
    EbPictureBufferDesc_t ref_picture[2];
    uint8_t *ref_mem[2];
    EbMemoryMapEntry map[64];
    uint32_t map_index;
    uint64_t lib_memory;
} G;

void drv_inloop_close(void)
{
    free(G.src), G.src = NULL;
    for (int l = 0; l < 2; l++) free(G.ref_mem[l]), G.ref_mem[l] = NULL;
}

int drv_inloop_open(int w, int h, int pad, const uint8_t *src, const uint8_t *ref0, const uint8_t *ref1)
{
    drv_inloop_close();
    if (!G.me) {   /* the context and the control sets live as long as the library */
        memoryMap = G.map, memoryMapIndex = &G.map_index, totalLibMemory = &G.lib_memory;
        if (in_loop_me_context_ctor(&G.me) != EB_ErrorNone) return -1;
        G.scs = (SequenceControlSet_t *)calloc(1, sizeof(*G.scs));
        G.enc = (EncodeContext_t *)calloc(1, sizeof(*G.enc));
        G.pcs = (PictureControlSet_t *)calloc(1, sizeof(*G.pcs));
        G.ppcs = (PictureParentControlSet_t *)calloc(1, sizeof(*G.ppcs));
        if (!G.scs || !G.enc || !G.pcs || !G.ppcs) return -1;
    }
    G.w = w, G.h = h, G.pad = pad, G.lists = ref1 ? 2 : 1;
    G.scs->luma_width = (uint16_t)w, G.scs->luma_height = (uint16_t)h;
    G.scs->sb_size = BLOCK_64X64, G.scs->sb_sz = 64;
    G.scs->static_config.encoder_bit_depth = EB_8BIT;
    G.scs->encode_context_ptr = G.enc;
    G.enc->asm_type = ASM_NON_AVX2;
    G.scs_wrapper.objectPtr = G.scs;
    G.pcs->sequence_control_set_wrapper_ptr = &G.scs_wrapper;
    G.pcs->parent_pcs_ptr = G.ppcs;
    G.pcs->slice_type = ref1 ? B_SLICE : P_SLICE;
    G.src = (uint8_t *)malloc((size_t)w * h);
    memcpy(G.src, src, (size_t)w * h);
    const uint8_t *refs[2] = {ref0, ref1};
    for (int l = 0; l < G.lists; l++) {
        EbPictureBufferDesc_t *d = &G.ref_picture[l];
        memset(d, 0, sizeof(*d));
        d->origin_x = d->origin_y = (uint16_t)pad;
        d->width = d->maxWidth = (uint16_t)w, d->height = d->maxHeight = (uint16_t)h;
        d->strideY = (uint16_t)(w + 2 * pad);
        d->lumaSize = (uint32_t)d->strideY * (h + 2 * pad);
        G.ref_mem[l] = (uint8_t *)malloc(d->lumaSize);   /* exactly the padded plane */
        memcpy(G.ref_mem[l], refs[l], d->lumaSize);
        d->bufferY = G.ref_mem[l];
        memset(&G.ref_object[l], 0, sizeof(G.ref_object[l]));
        G.ref_object[l].referencePicture = d;
        G.ref_wrapper[l].objectPtr = &G.ref_object[l];
        G.pcs->ref_pic_ptr_array[l] = &G.ref_wrapper[l];
    }
    return ((w + 63) / 64) * ((h + 63) / 64);
}

/* Codec/EbEncDecProcess.c:1509-1524 */
static void stage_superblock(int sb_x, int sb_y)
{
    const int sb_h = G.h - sb_y < 64 ? G.h - sb_y : 64, sb_w = G.w - sb_x < 64 ? G.w - sb_x : 64;
    memset(G.me->sb_buffer, 0, MAX_SB_SIZE * MAX_SB_SIZE);   /* the buffer's rows are MAX_SB_SIZE = 128 apart whatever the SB size is */
    for (int r = 0; r < sb_h; r++) memcpy(G.me->sb_buffer + r * MAX_SB_SIZE, G.src + (size_t)(sb_y + r) * G.w + sb_x, (size_t)sb_w);
    G.me->sb_src_ptr = G.me->sb_buffer;
    G.me->sb_src_stride = G.me->sb_buffer_stride;
}

int drv_inloop_run(int sb_x, int sb_y, const int16_t *center, int area_w, int area_h, int use_subpel, int prefill, int16_t *origin, uint32_t *sad,
                   uint32_t *mv, int16_t *inloop_mv)
{
    if (!G.src) return -1;
    stage_superblock(sb_x, sb_y);
    G.ppcs->use_subpel_flag = (uint8_t)use_subpel;
    G.me->search_area_width = (uint8_t)area_w, G.me->search_area_height = (uint8_t)area_h;
    memset(G.me->p_sb_best_sad, prefill, sizeof(G.me->p_sb_best_sad));
    memset(G.me->p_sb_best_mv, prefill, sizeof(G.me->p_sb_best_mv));
    memset(G.me->inloop_me_mv, prefill, sizeof(G.me->inloop_me_mv));
    {   /* the interpolated planes are malloc'ed, never cleared and reused from superblock to superblock (:3984-3996) */
        const size_t n = (size_t)G.me->interpolated_stride * MAX_SEARCH_AREA_HEIGHT;
        for (int l = 0; l < MAX_NUM_OF_REF_PIC_LIST; l++)
            memset(G.me->pos_b_buffer[l][0], prefill, n), memset(G.me->pos_h_buffer[l][0], prefill, n), memset(G.me->pos_j_buffer[l][0], prefill, n);
        memset(G.me->avctemp_buffer, prefill, n);
    }
    if (in_loop_motion_estimation_sblock(G.pcs, (uint32_t)sb_x, (uint32_t)sb_y, center[0], center[1], center[2], center[3], G.me) != EB_ErrorNone)
        return -2;
    for (int l = 0; l < G.lists; l++) {
        origin[2 * l] = G.me->x_search_area_origin[l][0], origin[2 * l + 1] = G.me->y_search_area_origin[l][0];
        memcpy(sad + (size_t)l * N_BLOCKS, G.me->p_sb_best_sad[l][0], sizeof(uint32_t) * N_BLOCKS);
        memcpy(mv + (size_t)l * N_BLOCKS, G.me->p_sb_best_mv[l][0], sizeof(uint32_t) * N_BLOCKS);
        memcpy(inloop_mv + (size_t)l * N_BLOCKS * 2, G.me->inloop_me_mv[l][0], sizeof(int16_t) * N_BLOCKS * 2);
    }
    return 0;
}

double drv_inloop_time(int area_w, int area_h, int use_subpel, int reps)
{
    struct timespec a, b;
    const int keep = (int)G.pcs->slice_type;
    G.pcs->slice_type = P_SLICE;
    G.ppcs->use_subpel_flag = (uint8_t)use_subpel;
    G.me->search_area_width = (uint8_t)area_w, G.me->search_area_height = (uint8_t)area_h;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int i = 0; i < reps; i++)
        for (int y = 0; y < G.h; y += 64)
            for (int x = 0; x < G.w; x += 64) {
                stage_superblock(x, y);
                in_loop_motion_estimation_sblock(G.pcs, (uint32_t)x, (uint32_t)y, 0, 0, 0, 0, G.me);
            }
    clock_gettime(CLOCK_MONOTONIC, &b);
    G.pcs->slice_type = keep;
    return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec);
}
