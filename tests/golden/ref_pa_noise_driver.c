/*
 * tests/golden/ref_pa_noise_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own FullSampleDenoise (Codec/EbPictureAnalysisProcess.c:3357-3410: the resets, DetectInputPictureNoise and, with
 * denoiseFlag, DenoiseInputPicture) for tests/golden/make_golden_pa_noise.py, tests/test_pa_noise_vs_ref.py and tools/pa_noise_probe.py
 * --cpu.  Contains no reference code: it builds the objects that function reads the way PictureAnalysisContextCtor (:44-90) and the
 * encoder do -- the input picture with 68 luma / 34 chroma border samples, a denoised picture of the same geometry whose Cb and Cr
 * pointers alias its luma buffer (bufferY, bufferY + chromaSize), a noise picture 64 rows high -- and calls it with asm_type ASM_AVX2
 * (as the encoder) or ASM_NON_AVX2 (the C function pointers), in either block_mean_calc_prec.
 *   drv_pa_noise_open     the three unpadded planes of a width x height picture; returns the number of SBs.  The borders of the input
 *                         picture are filled with 0xEE: nothing FullSampleDenoise leaves may depend on them
 *   drv_pa_noise_run      FullSampleDenoise on a fresh copy of the planes; copies out sb_flat_noise_array [n_sb], picture[4] =
 *                         sum of (noise variance >> 16) over complete SBs and their count (recovered exactly from picNoiseVarianceFloat,
 *                         a quotient of two small integers), pic_noise_class, picNoiseVarianceFloat >= 1.0; the denoised luma [h][w]
 *                         as DetectInputPictureNoise left it (before the chroma arm reuses the buffer); the three input planes afterwards
 *   drv_pa_noise_sb_var   [n_sb][2]: the reference's WeakLumaFilter / noiseExtractLumaWeak and ComputeVariance64x64 called SB row by SB
 *                         row on the same objects, for the two per-SB variances DetectInputPictureNoise does not keep (0 for incomplete SBs)
 *   drv_pa_noise_time     seconds of `reps` calls of FullSampleDenoise with denoiseFlag 0 (the CPU yardstick)
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbDefinitions.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbPictureAnalysisProcess.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

EbErrorType FullSampleDenoise(PictureAnalysisContext_t *context_ptr, SequenceControlSet_t *scs, PictureParentControlSet_t *pcs, uint32_t sb_total_count,
                              EbBool denoiseFlag, uint32_t picture_width_in_sb, EbAsm asm_type);
uint64_t ComputeVariance64x64(SequenceControlSet_t *scs, EbPictureBufferDesc_t *picture, uint32_t origin_index, uint64_t *variance32x32, EbAsm asm_type);

#define PAD 68

static struct {
    int w, h, nx, n_sb;
    SequenceControlSet_t *scs;
    PictureParentControlSet_t *pcs;
    PictureAnalysisContext_t ctx;
    EbPictureBufferDesc_t input, denoised, noise;
    uint8_t *mem[5], *planes[3];
} G;

void drv_pa_noise_close(void)
{
    if (!G.pcs) return;
    free(G.pcs->sb_flat_noise_array);
    for (int i = 0; i < 5; i++) free(G.mem[i]);
    for (int i = 0; i < 3; i++) free(G.planes[i]);
    free(G.scs); free(G.pcs);
    memset(&G, 0, sizeof(G));
}

static void luma_desc(EbPictureBufferDesc_t *d, int w, int h, uint8_t **mem)
{
    d->origin_x = d->origin_y = PAD;
    d->width = d->maxWidth = (uint16_t)w, d->height = d->maxHeight = (uint16_t)h;
    d->strideY = (uint16_t)(w + 2 * PAD), d->strideCb = d->strideCr = (uint16_t)(w / 2 + PAD);
    d->lumaSize = (uint32_t)d->strideY * (h + 2 * PAD), d->chromaSize = d->lumaSize >> 2;
    *mem = (uint8_t *)malloc(d->lumaSize);
    d->bufferY = *mem;
}

static void load_input(void)
{
    EbPictureBufferDesc_t *d = &G.input;
    memset(G.mem[0], 0xEE, d->lumaSize), memset(G.mem[1], 0xEE, d->chromaSize), memset(G.mem[2], 0xEE, d->chromaSize);
    for (int y = 0; y < G.h; y++) memcpy(d->bufferY + (size_t)(PAD + y) * d->strideY + PAD, G.planes[0] + (size_t)y * G.w, G.w);
    for (int y = 0; y < G.h / 2; y++) {
        memcpy(d->bufferCb + (size_t)(PAD / 2 + y) * d->strideCb + PAD / 2, G.planes[1] + (size_t)y * (G.w / 2), G.w / 2);
        memcpy(d->bufferCr + (size_t)(PAD / 2 + y) * d->strideCr + PAD / 2, G.planes[2] + (size_t)y * (G.w / 2), G.w / 2);
    }
    memset(G.mem[3], 0x55, G.denoised.lumaSize), memset(G.mem[4], 0x55, G.noise.lumaSize);
}

int drv_pa_noise_open(int w, int h, const uint8_t *luma, const uint8_t *cb, const uint8_t *cr)
{
    drv_pa_noise_close();
    G.w = w, G.h = h, G.nx = (w + 63) / 64, G.n_sb = G.nx * ((h + 63) / 64);
    G.scs = (SequenceControlSet_t *)calloc(1, sizeof(*G.scs));
    G.pcs = (PictureParentControlSet_t *)calloc(1, sizeof(*G.pcs));
    G.scs->sb_sz = 64;
    G.scs->luma_width = (uint16_t)w, G.scs->luma_height = (uint16_t)h;
    G.scs->chroma_width = (uint16_t)(w / 2), G.scs->chroma_height = (uint16_t)(h / 2);
    G.pcs->sb_flat_noise_array = (uint8_t *)calloc(G.n_sb, 1);
    G.pcs->sb_total_count = (uint16_t)G.n_sb;
    const uint8_t *src[3] = {luma, cb, cr};
    for (int i = 0; i < 3; i++) {
        const size_t n = (size_t)w * h / (i ? 4 : 1);
        G.planes[i] = (uint8_t *)malloc(n);
        memcpy(G.planes[i], src[i], n);
    }
    luma_desc(&G.input, w, h, &G.mem[0]);
    G.mem[1] = (uint8_t *)malloc(G.input.chromaSize), G.mem[2] = (uint8_t *)malloc(G.input.chromaSize);
    G.input.bufferCb = G.mem[1], G.input.bufferCr = G.mem[2];
    luma_desc(&G.denoised, w, h, &G.mem[3]);
    G.denoised.bufferCb = G.denoised.bufferY, G.denoised.bufferCr = G.denoised.bufferY + G.denoised.chromaSize;   /* as the constructor, :72-73 */
    luma_desc(&G.noise, w, 64, &G.mem[4]);
    G.noise.bufferCb = G.noise.bufferCr = NULL;
    G.pcs->enhanced_picture_ptr = &G.input;
    G.ctx.denoisedPicturePtr = &G.denoised, G.ctx.noisePicturePtr = &G.noise;
    return G.n_sb;
}

static void full_sample_denoise(int sub_precision, int denoise_flag, int avx2)
{
    G.scs->block_mean_calc_prec = sub_precision ? BLOCK_MEAN_PREC_SUB : BLOCK_MEAN_PREC_FULL;
    FullSampleDenoise(&G.ctx, G.scs, G.pcs, (uint32_t)G.n_sb, denoise_flag ? EB_TRUE : EB_FALSE, (uint32_t)G.nx, avx2 ? ASM_AVX2 : ASM_NON_AVX2);
}

int drv_pa_noise_run(int sub_precision, int denoise_flag, int avx2, uint8_t *flat_noise, uint32_t *picture, uint8_t *denoised, uint8_t *out_luma,
                     uint8_t *out_cb, uint8_t *out_cr)
{
    if (!G.pcs) return -1;
    load_input();
    /* the denoised luma is wanted as detection left it: run detection alone first, then the whole call on fresh planes */
    full_sample_denoise(sub_precision, 0, avx2);
    for (int y = 0; y < G.h; y++) memcpy(denoised + (size_t)y * G.w, G.denoised.bufferY + (size_t)(PAD + y) * G.denoised.strideY + PAD, G.w);
    if (denoise_flag) {
        load_input();
        full_sample_denoise(sub_precision, 1, avx2);
    }
    memcpy(flat_noise, G.pcs->sb_flat_noise_array, G.n_sb);
    uint32_t count = 0;
    for (int i = 0; i < G.n_sb; i++) count += (i % G.nx) * 64 + 64 <= G.w && (i / G.nx) * 64 + 64 <= G.h;
    picture[0] = (uint32_t)llround(G.ctx.picNoiseVarianceFloat * (double)count);
    picture[1] = count, picture[2] = (uint32_t)G.pcs->pic_noise_class, picture[3] = G.ctx.picNoiseVarianceFloat >= 1.0;
    const EbPictureBufferDesc_t *d = &G.input;
    for (int y = 0; y < G.h; y++) memcpy(out_luma + (size_t)y * G.w, d->bufferY + (size_t)(PAD + y) * d->strideY + PAD, G.w);
    for (int y = 0; y < G.h / 2; y++) {
        memcpy(out_cb + (size_t)y * (G.w / 2), d->bufferCb + (size_t)(PAD / 2 + y) * d->strideCb + PAD / 2, G.w / 2);
        memcpy(out_cr + (size_t)y * (G.w / 2), d->bufferCr + (size_t)(PAD / 2 + y) * d->strideCr + PAD / 2, G.w / 2);
    }
    /* no border byte of the input picture was written */
    for (int y = 0; y < G.h + 2 * PAD; y++)
        for (int x = 0; x < d->strideY; x++)
            if ((y < PAD || y >= PAD + G.h || x < PAD || x >= PAD + G.w) && d->bufferY[(size_t)y * d->strideY + x] != 0xEE) return -2;
    return 0;
}

int drv_pa_noise_sb_var(int sub_precision, int avx2, uint64_t *sb_var)
{
    if (!G.pcs) return -1;
    const EbAsm asm_type = avx2 ? ASM_AVX2 : ASM_NON_AVX2;
    load_input();
    G.scs->block_mean_calc_prec = sub_precision ? BLOCK_MEAN_PREC_SUB : BLOCK_MEAN_PREC_FULL;
    memset(sb_var, 0, (size_t)G.n_sb * 16);
    for (int i = 0; i < G.n_sb; i++) {
        const uint32_t x0 = (uint32_t)(i % G.nx) * 64, y0 = (uint32_t)(i / G.nx) * 64;
        uint64_t unused[4];
        if (x0 == 0) WeakLumaFilter_funcPtrArray[asm_type](&G.input, &G.denoised, &G.noise, y0, x0);
        if (x0 + 64 > (uint32_t)G.w) noiseExtractLumaWeak(&G.input, &G.denoised, &G.noise, y0, x0);
        if (x0 + 64 > (uint32_t)G.w || y0 + 64 > (uint32_t)G.h) continue;
        sb_var[2 * i] = ComputeVariance64x64(G.scs, &G.noise, PAD + x0 + (uint32_t)PAD * G.noise.strideY, unused, asm_type);
        sb_var[2 * i + 1] = ComputeVariance64x64(G.scs, &G.denoised, (PAD + y0) * G.denoised.strideY + PAD + x0, unused, asm_type) >> 16;
    }
    return 0;
}

double drv_pa_noise_time(int sub_precision, int reps)
{
    struct timespec a, b;
    load_input();
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int i = 0; i < reps; i++) full_sample_denoise(sub_precision, 0, 1);
    clock_gettime(CLOCK_MONOTONIC, &b);
    return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec);
}
