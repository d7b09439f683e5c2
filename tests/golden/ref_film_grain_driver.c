/*
 * tests/golden/ref_film_grain_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own film-grain synthesis for tests/golden/make_golden_film_grain.py, tests/test_film_grain_vs_ref.py and
 * tools/film_grain_probe.py --cpu.  Contains no reference code.  The templates and scaling tables are locals and file statics of
 * Codec/grainSynthesis.c, so this file includes that source where it lies (the link leaves grainSynthesis.o out) and calls its static
 * functions in the order av1_add_film_grain_run (:1014-1088) does.
 *   drv_fg_params_size / drv_fg_params_offsets   sizeof(aom_film_grain_t) and the offset of every field, in declaration order
 *   drv_fg_tables    luma [73][82], Cb, Cr [38][44] templates and the three 256-entry scaling tables as int32, as the reference's functions
 *                    leave them for `params` (params->bit_depth is read); a template of a plane without points is returned as zeros
 *   drv_fg_run       av1_add_film_grain_run in place on three w x h (w/2 x h/2) planes with the given strides (in samples)
 *   drv_fg_add       av1_add_film_grain (Codec/EbEncDecProcess.c:2001-2069) from a source into a destination EbPictureBufferDesc_t with
 *                    different borders; both are built here with every border sample 0xEE / 0xEEEE, and -2 is returned if a border
 *                    sample of either changed.  params->bit_depth is deliberately wrong on entry: the wrapper overwrites it
 *   drv_fg_time      seconds of `reps` calls of av1_add_film_grain on one thread (the CPU yardstick)
 * NEVER call any of these with num_y_points == 0: the reference's dealloc_arrays (:402-438) then frees one pointer more than init_arrays
 * allocated.  Every entry refuses that with -3.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbDefinitions.h"
#include "EbPictureBufferDesc.h"
#include "grainSynthesis.c"

void av1_add_film_grain(EbPictureBufferDesc_t *src, EbPictureBufferDesc_t *dst, aom_film_grain_t *film_grain_ptr);

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

#define LUMA_H 73
#define LUMA_W 82
#define CHROMA_H 38
#define CHROMA_W 44

int drv_fg_params_size(void) { return (int)sizeof(aom_film_grain_t); }

int drv_fg_params_offsets(int32_t *out)
{
#define O(f) out[n++] = (int32_t)offsetof(aom_film_grain_t, f)
    int n = 0;
    O(apply_grain); O(update_parameters); O(scaling_points_y); O(num_y_points); O(scaling_points_cb); O(num_cb_points); O(scaling_points_cr);
    O(num_cr_points); O(scaling_shift); O(ar_coeff_lag); O(ar_coeffs_y); O(ar_coeffs_cb); O(ar_coeffs_cr); O(ar_coeff_shift); O(cb_mult);
    O(cb_luma_mult); O(cb_offset); O(cr_mult); O(cr_luma_mult); O(cr_offset); O(overlap_flag); O(clip_to_restricted_range); O(bit_depth);
    O(chroma_scaling_from_luma); O(grain_scale_shift); O(random_seed);
#undef O
    return n;
}

int drv_fg_tables(const aom_film_grain_t *in, int32_t *luma, int32_t *cb, int32_t *cr, int32_t *scaling)
{
    aom_film_grain_t params = *in;
    int32_t **pos_luma, **pos_chroma, *yb, *cbb, *crb, *yl, *cbl, *crl, *yc, *cbc, *crc;
    if (params.num_y_points == 0) return -3;
    const int bd = params.bit_depth;
    random_register = params.random_seed;
    luma_subblock_size_y = luma_subblock_size_x = 32;
    chroma_subblock_size_y = chroma_subblock_size_x = 16;
    grain_center = 128 << (bd - 8);
    grain_min = 0 - grain_center;
    grain_max = (256 << (bd - 8)) - 1 - grain_center;
    init_arrays(&params, 64, 32, &pos_luma, &pos_chroma, &yb, &cbb, &crb, &yl, &cbl, &crl, &yc, &cbc, &crc, LUMA_H * LUMA_W, CHROMA_H * CHROMA_W, 1, 1);
    memset(yb, 0, sizeof(int32_t) * LUMA_H * LUMA_W);
    memset(cbb, 0, sizeof(int32_t) * CHROMA_H * CHROMA_W);
    memset(crb, 0, sizeof(int32_t) * CHROMA_H * CHROMA_W);
    generate_luma_grain_block(&params, pos_luma, yb, LUMA_H, LUMA_W, LUMA_W, 3, 3, 3, 0);
    generate_chroma_grain_blocks(&params, pos_chroma, yb, cbb, crb, LUMA_W, CHROMA_H, CHROMA_W, CHROMA_W, 3, 3, 3, 0, 1, 1);
    init_scaling_function(params.scaling_points_y, params.num_y_points, scaling_lut_y);
    if (params.chroma_scaling_from_luma) {
        memcpy(scaling_lut_cb, scaling_lut_y, sizeof(scaling_lut_y));
        memcpy(scaling_lut_cr, scaling_lut_y, sizeof(scaling_lut_y));
    } else {
        init_scaling_function(params.scaling_points_cb, params.num_cb_points, scaling_lut_cb);
        init_scaling_function(params.scaling_points_cr, params.num_cr_points, scaling_lut_cr);
    }
    memcpy(luma, yb, sizeof(int32_t) * LUMA_H * LUMA_W);
    memcpy(cb, cbb, sizeof(int32_t) * CHROMA_H * CHROMA_W);
    memcpy(cr, crb, sizeof(int32_t) * CHROMA_H * CHROMA_W);
    if (!params.num_cb_points) memset(cb, 0, sizeof(int32_t) * CHROMA_H * CHROMA_W);   /* multiplied into a discarded sum only */
    if (!params.num_cr_points) memset(cr, 0, sizeof(int32_t) * CHROMA_H * CHROMA_W);
    memcpy(scaling, scaling_lut_y, sizeof(scaling_lut_y));
    memcpy(scaling + 256, scaling_lut_cb, sizeof(scaling_lut_cb));
    memcpy(scaling + 512, scaling_lut_cr, sizeof(scaling_lut_cr));
    dealloc_arrays(&params, &pos_luma, &pos_chroma, &yb, &cbb, &crb, &yl, &cbl, &crl, &yc, &cbc, &crc);
    return 0;
}

int drv_fg_run(const aom_film_grain_t *in, void *luma, void *cb, void *cr, int w, int h, int luma_stride, int chroma_stride, int bit_depth)
{
    aom_film_grain_t params = *in;
    if (params.num_y_points == 0) return -3;
    params.bit_depth = bit_depth;
    av1_add_film_grain_run(&params, (uint8_t *)luma, (uint8_t *)cb, (uint8_t *)cr, h, w, luma_stride, chroma_stride, bit_depth > 8, 1, 1);
    return 0;
}

/* a picture buffer of w x h with borders ox, oy (luma samples, even), every sample 0xEE.. */
static void make_desc(EbPictureBufferDesc_t *d, int w, int h, int ox, int oy, int bit_depth)
{
    const int bytes = bit_depth > 8 ? 2 : 1;
    memset(d, 0, sizeof(*d));
    d->bit_depth = bit_depth > 8 ? EB_10BIT : EB_8BIT;
    d->origin_x = (uint16_t)ox, d->origin_y = (uint16_t)oy;
    d->width = d->maxWidth = (uint16_t)w, d->height = d->maxHeight = (uint16_t)h;
    d->strideY = (uint16_t)(w + 2 * ox), d->strideCb = d->strideCr = (uint16_t)(w / 2 + ox);
    d->lumaSize = (uint32_t)d->strideY * (h + 2 * oy), d->chromaSize = (uint32_t)d->strideCb * (h / 2 + oy);
    d->bufferY = (uint8_t *)malloc((size_t)d->lumaSize * bytes), d->bufferCb = (uint8_t *)malloc((size_t)d->chromaSize * bytes);
    d->bufferCr = (uint8_t *)malloc((size_t)d->chromaSize * bytes);
    memset(d->bufferY, 0xEE, (size_t)d->lumaSize * bytes);
    memset(d->bufferCb, 0xEE, (size_t)d->chromaSize * bytes), memset(d->bufferCr, 0xEE, (size_t)d->chromaSize * bytes);
}

static void free_desc(EbPictureBufferDesc_t *d) { free(d->bufferY), free(d->bufferCb), free(d->bufferCr); }

/* copies plane p of d from (to) a dense array; counts border bytes that are not 0xEE when `check` */
static int plane_io(EbPictureBufferDesc_t *d, int p, uint8_t *dense, int to_desc, int check, int bytes)
{
    uint8_t *buf = p == 0 ? d->bufferY : p == 1 ? d->bufferCb : d->bufferCr;
    const int stride = p == 0 ? d->strideY : d->strideCb, w = d->width >> (p > 0), h = d->height >> (p > 0);
    const int ox = d->origin_x >> (p > 0), oy = d->origin_y >> (p > 0), rows = (int)((p == 0 ? d->lumaSize : d->chromaSize) / stride);
    int bad = 0;
    for (int y = 0; y < h; y++) {
        uint8_t *row = buf + ((size_t)(oy + y) * stride + ox) * bytes;
        if (to_desc) memcpy(row, dense + (size_t)y * w * bytes, (size_t)w * bytes);
        else memcpy(dense + (size_t)y * w * bytes, row, (size_t)w * bytes);
    }
    if (check)
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < stride; x++)
                if (y < oy || y >= oy + h || x < ox || x >= ox + w)
                    for (int b = 0; b < bytes; b++) bad += buf[((size_t)y * stride + x) * bytes + b] != 0xEE;
    return bad;
}

int drv_fg_add(const aom_film_grain_t *in, int w, int h, int bit_depth, void *luma, void *cb, void *cr, void *out_luma, void *out_cb, void *out_cr)
{
    aom_film_grain_t params = *in;
    EbPictureBufferDesc_t src, dst;
    const int bytes = bit_depth > 8 ? 2 : 1;
    int bad = 0;
    if (params.num_y_points == 0) return -3;
    params.bit_depth = 12;   /* overwritten from the buffer by the wrapper (:2010-2030) */
    make_desc(&src, w, h, 68, 68, bit_depth);
    make_desc(&dst, w, h, 36, 12, bit_depth);
    void *ins[3] = {luma, cb, cr}, *outs[3] = {out_luma, out_cb, out_cr};
    for (int p = 0; p < 3; p++) plane_io(&src, p, (uint8_t *)ins[p], 1, 0, bytes);
    av1_add_film_grain(&src, &dst, &params);
    for (int p = 0; p < 3; p++) {
        bad += plane_io(&dst, p, (uint8_t *)outs[p], 0, 1, bytes);
        /* the source keeps what it held */
        uint8_t *again = (uint8_t *)malloc((size_t)w * h * bytes);
        bad += plane_io(&src, p, again, 0, 1, bytes);
        bad += memcmp(again, ins[p], (size_t)(w >> (p > 0)) * (h >> (p > 0)) * bytes) != 0;
        free(again);
    }
    free_desc(&src), free_desc(&dst);
    return bad ? -2 : 0;
}

double drv_fg_time(const aom_film_grain_t *in, int w, int h, int bit_depth, int reps)
{
    aom_film_grain_t params = *in;
    EbPictureBufferDesc_t src, dst;
    struct timespec a, b;
    if (params.num_y_points == 0) return -3.0;
    make_desc(&src, w, h, 68, 68, bit_depth);
    make_desc(&dst, w, h, 68, 68, bit_depth);
    for (size_t i = 0; i < (size_t)src.lumaSize * (bit_depth > 8 ? 2 : 1); i++) src.bufferY[i] = (uint8_t)(i * 2654435761u >> 24) & (bit_depth > 8 && (i & 1) ? 3 : 255);
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int i = 0; i < reps; i++) av1_add_film_grain(&src, &dst, &params);
    clock_gettime(CLOCK_MONOTONIC, &b);
    free_desc(&src), free_desc(&dst);
    return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec);
}
