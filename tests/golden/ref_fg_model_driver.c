/*
 * tests/golden/ref_fg_model_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own film-grain estimation (Codec/noise_model.c) for tests/golden/make_golden_fg_model.py,
 * tests/test_fg_model_vs_ref.py and tools/film_grain_model_probe.py --cpu.  Contains no reference code: aom_noise_model_init / _update /
 * _free and aom_flat_block_finder_init / _run / _extract_block / _free are called, and what they leave is copied out.
 *   drv_fgm_update    aom_noise_model_init (square shape, lag 3) + aom_noise_model_update on three planes of data and of denoised samples
 *                     (uint8_t, or uint16_t when bit_depth > 8; strides in samples, 4:2:0) with the given flat-block map; latest_state and
 *                     combined_state are copied into a svthip_film_grain_noise_state (include/svtav1_hip.h); returns the status
 *   drv_fgm_tables    A[1024][3] then AtA_inv[3][3] of aom_flat_block_finder_init(32, bit_depth)
 *   drv_fgm_flat_run  aom_flat_block_finder_run on a luma plane: the final map; returns its count of flat blocks
 *   drv_fgm_extract   aom_flat_block_finder_extract_block at (offsx, offsy): plane[1024] and block[1024]
 *   drv_fgm_time      seconds of `reps` calls of what = 0: aom_noise_model_init + _update + _free, 1: aom_flat_block_finder_run (one thread)
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbDefinitions.h"
#include "noise_model.h"
#include "svtav1_hip.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

#define BLOCK 32

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

static int update(int bit_depth, int w, int h, const uint8_t *const data[3], const uint8_t *const den[3], int stride[3], const uint8_t *flat,
                  svthip_film_grain_noise_state *out)
{
    const aom_noise_model_params_t params = {AOM_NOISE_SHAPE_SQUARE, 3, bit_depth, bit_depth > 8};
    int chroma_sub_log2[2] = {1, 1};
    aom_noise_model_t model;
    int status, c;
    if (!aom_noise_model_init(&model, params)) return -1;
    status = (int)aom_noise_model_update(&model, data, den, w, h, stride, chroma_sub_log2, flat, BLOCK);
    if (out) {
        memset(out, 0, sizeof(*out));
        for (c = 0; c < 3; c++) {
            if (model.latest_state[c].eqns.n > SVTHIP_FILM_GRAIN_NOISE_MAX_COEFFS || model.latest_state[c].strength_solver.num_bins != SVTHIP_FILM_GRAIN_NOISE_BINS)
                return -2;
            copy_state(&out->latest[c], &model.latest_state[c]);
            copy_state(&out->combined[c], &model.combined_state[c]);
        }
        out->status = status;
    }
    aom_noise_model_free(&model);
    return status;
}

int drv_fgm_state_size(void) { return (int)sizeof(svthip_film_grain_noise_state); }

int drv_fgm_update(int bit_depth, int w, int h, const void *d0, const void *d1, const void *d2, const void *n0, const void *n1, const void *n2, int s0,
                   int s1, int s2, const uint8_t *flat, svthip_film_grain_noise_state *out)
{
    const uint8_t *const data[3] = {d0, d1, d2}, *const den[3] = {n0, n1, n2};
    int stride[3] = {s0, s1, s2};
    return update(bit_depth, w, h, data, den, stride, flat, out);
}

int drv_fgm_tables(int bit_depth, double *out)
{
    aom_flat_block_finder_t finder;
    if (!aom_flat_block_finder_init(&finder, BLOCK, bit_depth, bit_depth > 8)) return -1;
    memcpy(out, finder.A, sizeof(double) * BLOCK * BLOCK * 3);
    memcpy(out + BLOCK * BLOCK * 3, finder.AtA_inv, sizeof(double) * 9);
    aom_flat_block_finder_free(&finder);
    return 0;
}

int drv_fgm_flat_run(int bit_depth, const void *data, int w, int h, int stride, uint8_t *flat)
{
    aom_flat_block_finder_t finder;
    int n;
    if (!aom_flat_block_finder_init(&finder, BLOCK, bit_depth, bit_depth > 8)) return -1;
    n = aom_flat_block_finder_run(&finder, data, w, h, stride, flat);
    aom_flat_block_finder_free(&finder);
    return n;
}

int drv_fgm_extract(int bit_depth, const void *data, int w, int h, int stride, int offsx, int offsy, double *plane, double *block)
{
    aom_flat_block_finder_t finder;
    if (!aom_flat_block_finder_init(&finder, BLOCK, bit_depth, bit_depth > 8)) return -1;
    aom_flat_block_finder_extract_block(&finder, data, w, h, stride, offsx, offsy, plane, block);
    aom_flat_block_finder_free(&finder);
    return 0;
}

double drv_fgm_time(int what, int reps, int bit_depth, int w, int h, const void *d0, const void *d1, const void *d2, const void *n0, const void *n1,
                    const void *n2, int s0, int s1, int s2, uint8_t *flat)
{
    const uint8_t *const data[3] = {d0, d1, d2}, *const den[3] = {n0, n1, n2};
    int stride[3] = {s0, s1, s2}, r;
    struct timespec t0, t1;
    uint8_t *scratch = malloc((size_t)((w + BLOCK - 1) / BLOCK) * ((h + BLOCK - 1) / BLOCK));
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (r = 0; r < reps; r++) {
        if (what == 0)
            update(bit_depth, w, h, data, den, stride, flat, NULL);
        else
            drv_fgm_flat_run(bit_depth, d0, w, h, s0, scratch);
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    free(scratch);
    return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}
