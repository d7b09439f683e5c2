/*
 * tests/golden/ref_fg_denoise_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own film-grain Wiener denoising (Codec/noise_model.c, noise_util.c, fft.c) for
 * tests/golden/make_golden_fg_denoise.py, tests/test_fg_denoise_vs_ref.py and tools/film_grain_denoise_probe.py --cpu.  Contains no
 * reference code: the functions are called and what they leave is copied out.  The FFT pointers are the ones setup_rtcd_internal stores on
 * an AVX2 host (the encoder's dispatch, Codec/aom_dsp_rtcd.h:3061-3070).
 *   drv_fgd_denoise   aom_wiener_denoise_2d on three planes (uint8_t, or uint16_t when bit_depth > 8; strides in samples, 4:2:0), block 32
 *   drv_fgd_fft       aom_fft{16x16,32x32}_float through the dispatch pointer: the 2 n n floats of the spectrum
 *   drv_fgd_ifft      aom_ifft{16x16,32x32}_float through the dispatch pointer on 2 n n floats: n n floats
 *   drv_fgd_tx        aom_noise_tx_forward + _filter + _inverse on one block of n n floats with the given psd, in place
 *   drv_fgd_extract   aom_flat_block_finder_extract_block at block size n (16 or 32) and (offsx, offsy): plane[n n] and block[n n]
 *   drv_fgd_psd       aom_noise_psd_get_default_value
 *   drv_fgd_chain     aom_flat_block_finder_run + aom_wiener_denoise_2d + aom_noise_model_init / _update as aom_denoise_and_model_run
 *                     strings them, the psd flat at the default value of noise_level; the denoised planes, the map and the state
 *   drv_fgd_time      seconds of `reps` calls of aom_wiener_denoise_2d (one thread)
 */
#define RTCD_C
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbDefinitions.h"
#include "noise_model.h"
#include "noise_util.h"
#include "aom_dsp_rtcd.h"
#include "svtav1_hip.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

#define BLOCK 32

static void dispatch(void)
{
    static int done;
    if (!done) setup_rtcd_internal(ASM_AVX2);
    done = 1;
}

int drv_fgd_denoise(int bit_depth, int w, int h, const void *d0, const void *d1, const void *d2, void *n0, void *n1, void *n2, int s0, int s1, int s2,
                    float *psd0, float *psd1, float *psd2)
{
    const uint8_t *const data[3] = {d0, d1, d2};
    uint8_t *den[3] = {n0, n1, n2};
    int stride[3] = {s0, s1, s2}, chroma_sub[2] = {1, 1};
    float *psd[3] = {psd0, psd1, psd2};
    dispatch();
    return aom_wiener_denoise_2d(data, den, w, h, stride, chroma_sub, psd, BLOCK, bit_depth, bit_depth > 8);
}

static void *aligned32(size_t bytes)
{
    void *p = NULL;
    return posix_memalign(&p, 32, bytes) ? NULL : p;
}

int drv_fgd_fft(int n, const float *in, float *out)
{
    float *a = aligned32(sizeof(float) * n * n), *t = aligned32(sizeof(float) * 2 * n * n), *o = aligned32(sizeof(float) * 2 * n * n);
    dispatch();
    if (!a || !t || !o || (n != 16 && n != 32)) return -1;
    memcpy(a, in, sizeof(float) * n * n);
    memset(t, 0, sizeof(float) * 2 * n * n);
    memset(o, 0, sizeof(float) * 2 * n * n);
    (n == 32 ? aom_fft32x32_float : aom_fft16x16_float)(a, t, o);
    memcpy(out, o, sizeof(float) * 2 * n * n);
    free(a), free(t), free(o);
    return 0;
}

int drv_fgd_ifft(int n, const float *in, float *out)
{
    float *a = aligned32(sizeof(float) * 2 * n * n), *t = aligned32(sizeof(float) * 2 * n * n), *o = aligned32(sizeof(float) * n * n);
    dispatch();
    if (!a || !t || !o || (n != 16 && n != 32)) return -1;
    memcpy(a, in, sizeof(float) * 2 * n * n);
    memset(t, 0, sizeof(float) * 2 * n * n);
    (n == 32 ? aom_ifft32x32_float : aom_ifft16x16_float)(a, t, o);
    memcpy(out, o, sizeof(float) * n * n);
    free(a), free(t), free(o);
    return 0;
}

int drv_fgd_tx(int n, float *block, const float *psd)
{
    struct aom_noise_tx_t *tx;
    float *a = aligned32(sizeof(float) * n * n);
    dispatch();
    tx = aom_noise_tx_malloc(n);
    if (!tx || !a) return -1;
    memcpy(a, block, sizeof(float) * n * n);
    aom_noise_tx_forward(tx, a);
    aom_noise_tx_filter(tx, psd);
    aom_noise_tx_inverse(tx, a);
    memcpy(block, a, sizeof(float) * n * n);
    aom_noise_tx_free(tx);
    free(a);
    return 0;
}

int drv_fgd_extract(int bit_depth, int n, const void *data, int w, int h, int stride, int offsx, int offsy, double *plane, double *block)
{
    aom_flat_block_finder_t finder;
    if (!aom_flat_block_finder_init(&finder, n, bit_depth, bit_depth > 8)) return -1;
    aom_flat_block_finder_extract_block(&finder, data, w, h, stride, offsx, offsy, plane, block);
    aom_flat_block_finder_free(&finder);
    return 0;
}

float drv_fgd_psd(int block_size, float factor) { return aom_noise_psd_get_default_value(block_size, factor); }

static void copy_state(svthip_film_grain_noise_channel *out, const aom_noise_state_t *in)
{
    const int n = in->eqns.n, bins = in->strength_solver.num_bins;
    memset(out, 0, sizeof(*out));
    memcpy(out->A, in->eqns.A, sizeof(double) * n * n);
    memcpy(out->b, in->eqns.b, sizeof(double) * n);
    memcpy(out->x, in->eqns.x, sizeof(double) * n);
    out->ar_gain = in->ar_gain;
    memcpy(out->strength_A, in->strength_solver.eqns.A, sizeof(double) * bins * bins);
    memcpy(out->strength_b, in->strength_solver.eqns.b, sizeof(double) * bins);
    memcpy(out->strength_x, in->strength_solver.eqns.x, sizeof(double) * bins);
    out->strength_total = in->strength_solver.total;
    out->strength_num_equations = in->strength_solver.num_equations;
    out->num_observations = in->num_observations;
}

int drv_fgd_chain(int bit_depth, int w, int h, const void *d0, const void *d1, const void *d2, void *n0, void *n1, void *n2, int s0, int s1, int s2,
                  float noise_level, uint8_t *flat, svthip_film_grain_noise_state *out)
{
    const aom_noise_model_params_t params = {AOM_NOISE_SHAPE_SQUARE, 3, bit_depth, bit_depth > 8};
    const uint8_t *const data[3] = {d0, d1, d2};
    uint8_t *den[3] = {n0, n1, n2};
    int stride[3] = {s0, s1, s2}, chroma_sub[2] = {1, 1}, c, i, status;
    float *psd[3];
    aom_flat_block_finder_t finder;
    aom_noise_model_t model;
    dispatch();
    for (c = 0; c < 3; c++) {
        const float v = aom_noise_psd_get_default_value(BLOCK >> (c > 0), noise_level);
        psd[c] = malloc(sizeof(float) * BLOCK * BLOCK);
        for (i = 0; i < BLOCK * BLOCK; i++) psd[c][i] = v;
    }
    if (!aom_flat_block_finder_init(&finder, BLOCK, bit_depth, bit_depth > 8)) return -1;
    aom_flat_block_finder_run(&finder, data[0], w, h, stride[0], flat);
    aom_flat_block_finder_free(&finder);
    if (!aom_wiener_denoise_2d(data, den, w, h, stride, chroma_sub, psd, BLOCK, bit_depth, bit_depth > 8)) return -1;
    if (!aom_noise_model_init(&model, params)) return -1;
    status = (int)aom_noise_model_update(&model, data, (const uint8_t *const *)den, w, h, stride, chroma_sub, flat, BLOCK);
    memset(out, 0, sizeof(*out));
    for (c = 0; c < 3; c++) {
        copy_state(&out->latest[c], &model.latest_state[c]);
        copy_state(&out->combined[c], &model.combined_state[c]);
        free(psd[c]);
    }
    out->status = status;
    aom_noise_model_free(&model);
    return status;
}

double drv_fgd_time(int reps, int bit_depth, int w, int h, const void *d0, const void *d1, const void *d2, void *n0, void *n1, void *n2, int s0, int s1,
                    int s2, float *psd0, float *psd1, float *psd2)
{
    struct timespec t0, t1;
    int r;
    dispatch();
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (r = 0; r < reps; r++) drv_fgd_denoise(bit_depth, w, h, d0, d1, d2, n0, n1, n2, s0, s1, s2, psd0, psd1, psd2);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}
