/*
 * tests/golden/ref_cdef128_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own CDEF strength search, strength pick and frame filter on a mode-info grid that carries block sizes, for
 * tests/golden/make_golden_cdef128.py and tests/test_cdef128_vs_ref.py.  Contains no reference code: it builds the objects
 * cdef_seg_search[16bit], finish_cdef_search and av1_cdef_frame[16bit] read, as tests/golden/ref_cdef_driver.c does, and calls them, with
 * setup_rtcd_internal(ASM_AVX2) as the encoder and mse_4x4_16bit set back to its C form (see there).  The grid has sb_type, skip and
 * cdef_strength per cell; its rows and its stride are the picture's rounded up to 32 cells plus 32, so that the copies finish_cdef_search
 * makes for a 128-wide block at the picture's edge land in allocated cells.
 *   drv_cdef128_open     the deblocked and source planes, the skip map and the sb_type map (one byte per 4x4 luma cell, mi_rows x mi_cols)
 *   drv_cdef128_search   cdef_seg_search[16bit] as one segment: mse[2][nfb][64] (entries of fbs left out stay 0)
 *   drv_cdef128_finish   finish_cdef_search: res[21] as ref_cdef_driver.c, with sb_count = the fbs that are neither twins nor all skipped
 *                        (the reference keeps its count in a local); fb_strength[nfb] = cdef_strength of each fb's first cell, -1 before
 *   drv_cdef128_frame    av1_cdef_frame[16bit] on a copy of the deblocked planes with the strengths, dampings and per-fb indices given;
 *                        an index of -1 stays -1 (the reference passes such an fb over)
 */
#define RTCD_C
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "EbDefinitions.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbEncDecProcess.h"
#include "EbCdef.h"
#include "aom_dsp_rtcd.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

void cdef_seg_search(PictureControlSet_t *pcs, SequenceControlSet_t *scs, uint32_t segment_index);
void cdef_seg_search16bit(PictureControlSet_t *pcs, SequenceControlSet_t *scs, uint32_t segment_index);
void finish_cdef_search(EncDecContext_t *ctx, SequenceControlSet_t *scs, PictureControlSet_t *pcs);
void av1_cdef_frame(EncDecContext_t *ctx, SequenceControlSet_t *scs, PictureControlSet_t *pcs);
void av1_cdef_frame16bit(EncDecContext_t *ctx, SequenceControlSet_t *scs, PictureControlSet_t *pcs);

#define MARGIN 32

typedef struct {
    EbPictureBufferDesc_t d;
    uint8_t *mem[3];
} Pic;

static struct {
    int w, h, bd, nhfb, nvfb, mi_rows, mi_cols, mi_stride, grid_rows;
    PictureControlSet_t *pcs;
    PictureParentControlSet_t *ppcs;
    SequenceControlSet_t *scs;
    Av1Common *cm;
    ModeInfo *cell;
    ModeInfo **grid;
    Pic recon, source;
    void *dbk[3];
    uint16_t *src16[3], *ref16[3];
} G;

static void dispatch(void)
{
    setup_rtcd_internal(ASM_AVX2);
    mse_4x4_16bit = mse_4x4_16bit_c;
}

static size_t plane_off(int i) { const int m = i ? MARGIN / 2 : MARGIN, s = (i ? G.w / 2 : G.w) + 2 * m; return (size_t)m * s + m; }
static int plane_stride(int i) { return (i ? G.w / 2 : G.w) + 2 * (i ? MARGIN / 2 : MARGIN); }

static void pic_init(Pic *p)
{
    const int b = G.bd > 8 ? 2 : 1;
    memset(p, 0, sizeof(*p));
    p->d.origin_x = p->d.origin_y = MARGIN;
    p->d.width = p->d.maxWidth = (uint16_t)G.w;
    p->d.height = p->d.maxHeight = (uint16_t)G.h;
    p->d.bit_depth = (EB_BITDEPTH)G.bd;
    p->d.strideY = (uint16_t)plane_stride(0);
    p->d.strideCb = p->d.strideCr = (uint16_t)plane_stride(1);
    for (int i = 0; i < 3; i++) p->mem[i] = (uint8_t *)calloc((size_t)plane_stride(i) * ((i ? G.h / 2 : G.h) + 2 * MARGIN) + 64, b);
    p->d.bufferY = p->mem[0];
    p->d.bufferCb = p->mem[1];
    p->d.bufferCr = p->mem[2];
}

static void pic_copy(Pic *p, void *const planes[3], int out)
{
    const int b = G.bd > 8 ? 2 : 1;
    for (int i = 0; i < 3; i++) {
        const int pw = i ? G.w / 2 : G.w, ph = i ? G.h / 2 : G.h;
        for (int y = 0; y < ph; y++) {
            uint8_t *in_pic = p->mem[i] + (plane_off(i) + (size_t)y * plane_stride(i)) * b, *row = (uint8_t *)planes[i] + (size_t)y * pw * b;
            if (out) memcpy(row, in_pic, (size_t)pw * b); else memcpy(in_pic, row, (size_t)pw * b);
        }
    }
}

void drv_cdef128_close(void)
{
    if (!G.pcs) return;
    for (int i = 0; i < 3; i++) {
        free(G.recon.mem[i]); free(G.source.mem[i]);
        if (G.bd == 8) { free(G.src16[i]); free(G.ref16[i]); }
    }
    free(G.pcs->mse_seg[0]); free(G.pcs->mse_seg[1]);
    free(G.grid); free(G.cell); free(G.cm); free(G.scs); free(G.ppcs); free(G.pcs);
    memset(&G, 0, sizeof(G));
}

int drv_cdef128_open(int w, int h, int bd, void *const dbk[3], void *const src[3], const uint8_t *skip, const uint8_t *sb_type)
{
    drv_cdef128_close();
    dispatch();
    G.w = w, G.h = h, G.bd = bd;
    G.mi_cols = w >> 2, G.mi_rows = h >> 2;
    G.nhfb = (G.mi_cols + 15) / 16, G.nvfb = (G.mi_rows + 15) / 16;
    G.mi_stride = (G.mi_cols + 31) / 32 * 32 + 32;
    G.grid_rows = (G.mi_rows + 31) / 32 * 32 + 32;
    G.pcs = (PictureControlSet_t *)calloc(1, sizeof(*G.pcs));
    G.ppcs = (PictureParentControlSet_t *)calloc(1, sizeof(*G.ppcs));
    G.scs = (SequenceControlSet_t *)calloc(1, sizeof(*G.scs));
    G.cm = (Av1Common *)calloc(1, sizeof(*G.cm));
    const size_t cells = (size_t)G.grid_rows * G.mi_stride;
    G.cell = (ModeInfo *)calloc(cells, sizeof(*G.cell));
    G.grid = (ModeInfo **)calloc(cells, sizeof(*G.grid));
    for (size_t i = 0; i < cells; i++) {
        G.cell[i].mbmi.sb_type = BLOCK_8X8;
        G.cell[i].mbmi.skip = 1;
        G.cell[i].mbmi.cdef_strength = -1;
        G.grid[i] = &G.cell[i];
    }
    for (int r = 0; r < G.mi_rows; r++)
        for (int c = 0; c < G.mi_cols; c++) {
            G.cell[(size_t)r * G.mi_stride + c].mbmi.skip = skip[(size_t)r * G.mi_cols + c] != 0;
            G.cell[(size_t)r * G.mi_stride + c].mbmi.sb_type = (BlockSize)sb_type[(size_t)r * G.mi_cols + c];
        }
    pic_init(&G.recon);
    pic_init(&G.source);
    pic_copy(&G.recon, dbk, 0);
    pic_copy(&G.source, src, 0);
    for (int i = 0; i < 3; i++) G.dbk[i] = dbk[i];
    G.scs->static_config.encoder_bit_depth = (uint32_t)bd;
    G.scs->sb_size = BLOCK_128X128;
    G.scs->sb_size_pix = 128;
    G.scs->luma_width = (uint16_t)w;
    G.scs->luma_height = (uint16_t)h;
    G.scs->chroma_width = (uint16_t)(w / 2);
    G.scs->chroma_height = (uint16_t)(h / 2);
    G.cm->mi_rows = G.mi_rows, G.cm->mi_cols = G.mi_cols, G.cm->mi_stride = G.mi_stride;
    G.ppcs->av1_cm = G.cm;
    G.ppcs->sequence_control_set_ptr = G.scs;
    G.ppcs->is_used_as_reference_flag = EB_FALSE;
    G.ppcs->enhanced_picture_ptr = &G.source.d;
    G.pcs->parent_pcs_ptr = G.ppcs;
    G.pcs->mi_grid_base = G.grid;
    G.pcs->mi_stride = G.mi_stride;
    G.pcs->recon_picture_ptr = G.pcs->recon_picture16bit_ptr = &G.recon.d;
    G.pcs->input_frame16bit = &G.source.d;
    G.pcs->cdef_segments_column_count = G.pcs->cdef_segments_row_count = 1;
    G.pcs->cdef_segments_total_count = 1;
    for (int k = 0; k < 2; k++) G.pcs->mse_seg[k] = (uint64_t(*)[TOTAL_STRENGTHS])calloc((size_t)G.nhfb * G.nvfb, sizeof(uint64_t) * TOTAL_STRENGTHS);
    for (int i = 0; i < 3; i++) {
        const int pw = i ? w / 2 : w, ph = i ? h / 2 : h;
        if (bd > 8) {   /* EbDlfProcess.c:195-202 */
            G.src16[i] = (uint16_t *)G.recon.mem[i] + plane_off(i);
            G.ref16[i] = (uint16_t *)G.source.mem[i] + plane_off(i);
        } else {        /* :217-231: packed 16-bit copies */
            G.src16[i] = (uint16_t *)calloc((size_t)pw * ph, 2);
            G.ref16[i] = (uint16_t *)calloc((size_t)pw * ph, 2);
            for (size_t k = 0; k < (size_t)pw * ph; k++) G.src16[i][k] = ((const uint8_t *)dbk[i])[k], G.ref16[i][k] = ((const uint8_t *)src[i])[k];
        }
        G.pcs->src[i] = G.src16[i];
        G.pcs->ref_coeff[i] = G.ref16[i];
    }
    return G.nhfb * G.nvfb;
}

static void run_search(int base_qindex)
{
    G.ppcs->base_qindex = (uint8_t)base_qindex;
    for (int k = 0; k < 2; k++) memset(G.pcs->mse_seg[k], 0, (size_t)G.nhfb * G.nvfb * sizeof(uint64_t) * TOTAL_STRENGTHS);
    if (G.bd > 8) cdef_seg_search16bit(G.pcs, G.scs, 0); else cdef_seg_search(G.pcs, G.scs, 0);
}

int drv_cdef128_search(int base_qindex, uint64_t *mse)
{
    const size_t n = (size_t)G.nhfb * G.nvfb * TOTAL_STRENGTHS;
    pic_copy(&G.recon, G.dbk, 0);
    run_search(base_qindex);
    memcpy(mse, G.pcs->mse_seg[0], n * 8);
    memcpy(mse + n, G.pcs->mse_seg[1], n * 8);
    return 0;
}

static ModeInfo *fb_cell(int fb) { return G.grid[(size_t)(fb / G.nhfb) * 16 * G.mi_stride + (size_t)(fb % G.nhfb) * 16]; }

/* mse (may be null): tables to pick from instead of the last search's */
int drv_cdef128_finish(int base_qindex, const uint64_t *mse, int32_t *res, int8_t *fb_strength)
{
    const int nfb = G.nhfb * G.nvfb;
    const size_t n = (size_t)nfb * TOTAL_STRENGTHS;
    G.ppcs->base_qindex = (uint8_t)base_qindex;
    if (mse) memcpy(G.pcs->mse_seg[0], mse, n * 8), memcpy(G.pcs->mse_seg[1], mse + n, n * 8);
    for (size_t i = 0; i < (size_t)G.grid_rows * G.mi_stride; i++) G.cell[i].mbmi.cdef_strength = -1;
    int count = 0;
    finish_cdef_search(NULL, G.scs, G.pcs);
    res[0] = G.ppcs->cdef_bits, res[1] = G.ppcs->nb_cdef_strengths;
    for (int i = 0; i < 8; i++) res[2 + i] = i < res[1] ? G.ppcs->cdef_strengths[i] : 0, res[10 + i] = i < res[1] ? G.ppcs->cdef_uv_strengths[i] : 0;
    res[18] = G.ppcs->cdef_pri_damping, res[19] = G.ppcs->cdef_sec_damping;
    for (int fb = 0; fb < nfb; fb++) {
        const int fbr = fb / G.nhfb, fbc = fb % G.nhfb, t = fb_cell(fb)->mbmi.sb_type;
        int all_skip = 1;
        for (int r = 16 * fbr; r < 16 * fbr + 16 && r < G.mi_rows; r++)
            for (int c = 16 * fbc; c < 16 * fbc + 16 && c < G.mi_cols; c++) all_skip &= G.cell[(size_t)r * G.mi_stride + c].mbmi.skip != 0;
        const int twin = ((fbc & 1) && (t == BLOCK_128X128 || t == BLOCK_128X64)) || ((fbr & 1) && (t == BLOCK_128X128 || t == BLOCK_64X128));
        count += !twin && !all_skip;
        fb_strength[fb] = fb_cell(fb)->mbmi.cdef_strength;
    }
    res[20] = count;
    return 0;
}

static void run_frame(const int32_t *res, const int8_t *fb_strength)
{
    for (int i = 0; i < 8; i++) G.ppcs->cdef_strengths[i] = res[2 + i], G.ppcs->cdef_uv_strengths[i] = res[10 + i];
    G.ppcs->cdef_bits = res[0], G.ppcs->nb_cdef_strengths = res[1];
    G.ppcs->cdef_pri_damping = res[18], G.ppcs->cdef_sec_damping = res[19];
    /* -1 stays: av1_cdef_frame passes such an fb over (and says so), also where a wide fb left out has listed blocks in its other quadrants */
    for (int fb = 0; fb < G.nhfb * G.nvfb; fb++) fb_cell(fb)->mbmi.cdef_strength = fb_strength[fb];
    if (G.bd > 8) av1_cdef_frame16bit(NULL, G.scs, G.pcs); else av1_cdef_frame(NULL, G.scs, G.pcs);
}

int drv_cdef128_frame(const int32_t *res, const int8_t *fb_strength, void *const out[3])
{
    pic_copy(&G.recon, G.dbk, 0);
    run_frame(res, fb_strength);
    pic_copy(&G.recon, out, 1);
    pic_copy(&G.recon, G.dbk, 0);
    return 0;
}

