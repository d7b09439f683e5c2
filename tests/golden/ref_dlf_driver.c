/*
 * tests/golden/ref_dlf_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own deblocking filter and filter-level search for tests/golden/make_golden_dlf.py and tests/test_dlf_vs_ref.py.
 * Contains no reference code: it builds the few objects av1_loop_filter_frame, PictureSseCalculations and av1_pick_filter_level read (a
 * picture control set with its parent and sequence control set, the mode-info grid, picture descriptors over padded copies of the
 * caller's planes, a DlfContext_t with the scratch picture) and calls them.
 *   drv_dlf op 0   av1_loop_filter_frame(recon, pcs, plane_start, plane_end) with the four levels and the sharpness given
 *           op 1   av1_pick_filter_level(ctx, source, pcs, LPF_PICK_FROM_FULL_IMAGE) with levels[] as the last frame's; the levels it
 *                  leaves are returned.  trace[][4] receives the four levels of every av1_loop_filter_frame call it makes, in order
 *           op 2   op 0 on one plane, then PictureSseCalculations(pcs, recon, plane) into *sse
 * The trace is taken in Log2f_SSE2, which av1_loop_filter_frame calls once (EbDeblockingFilter.c:1470) and which the link does not have
 * (it is NASM code): the stand-in below answers the logarithm and notes the levels of the picture being filtered.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "EbDefinitions.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbDeblockingFilter.h"
#include "EbDlfProcess.h"

#define MARGIN 32

extern uint64_t PictureSseCalculations(PictureControlSet_t *picture_control_set_ptr, EbPictureBufferDesc_t *reconPtr, int32_t plane);

static struct {
    PictureControlSet_t *pcs;
    int32_t (*trace)[4];
    int n_trace, cap;
} G;

uint32_t Log2f_SSE2(uint32_t x)
{
    if (G.pcs && G.trace && G.n_trace < G.cap) {
        const struct loopfilter *lf = &G.pcs->parent_pcs_ptr->lf;
        int32_t *t = G.trace[G.n_trace];
        t[0] = lf->filter_level[0]; t[1] = lf->filter_level[1]; t[2] = lf->filter_level_u; t[3] = lf->filter_level_v;
    }
    G.n_trace++;
    return (uint32_t)(31 - __builtin_clz(x | 1));
}

typedef struct {
    EbPictureBufferDesc_t d;
    uint8_t *mem[3];
} Pic;

static void pic_init(Pic *p, int w, int h, int bd, void *const planes[3])
{
    const int b = bd > 8 ? 2 : 1;
    memset(p, 0, sizeof(*p));
    p->d.origin_x = p->d.origin_y = MARGIN;
    p->d.width = p->d.maxWidth = (uint16_t)w;
    p->d.height = p->d.maxHeight = (uint16_t)h;
    p->d.bit_depth = (EB_BITDEPTH)bd;
    p->d.strideY = (uint16_t)(w + 2 * MARGIN);
    p->d.strideCb = p->d.strideCr = (uint16_t)(w / 2 + MARGIN);
    for (int i = 0; i < 3; i++) {
        const int pw = i ? w / 2 : w, ph = i ? h / 2 : h, m = i ? MARGIN / 2 : MARGIN, s = pw + 2 * m;
        p->mem[i] = (uint8_t *)calloc((size_t)s * (ph + 2 * m) + 64, b);
        if (planes)
            for (int y = 0; y < ph; y++) memcpy(p->mem[i] + ((size_t)(y + m) * s + m) * b, (const uint8_t *)planes[i] + (size_t)y * pw * b, (size_t)pw * b);
    }
    p->d.bufferY = p->mem[0];
    p->d.bufferCb = p->mem[1];
    p->d.bufferCr = p->mem[2];
}

static void pic_out(const Pic *p, int w, int h, int bd, void *const planes[3])
{
    const int b = bd > 8 ? 2 : 1;
    for (int i = 0; i < 3; i++) {
        const int pw = i ? w / 2 : w, ph = i ? h / 2 : h, m = i ? MARGIN / 2 : MARGIN, s = pw + 2 * m;
        for (int y = 0; y < ph; y++) memcpy((uint8_t *)planes[i] + (size_t)y * pw * b, p->mem[i] + ((size_t)(y + m) * s + m) * b, (size_t)pw * b);
    }
}

static void pic_free(Pic *p)
{
    for (int i = 0; i < 3; i++) free(p->mem[i]);
}

/* mi: mi_rows x mi_stride cells of 4 bytes (sb_type, tx_size, flags, reserved), mi_stride = 16 * superblock columns */
int drv_dlf(int op, int w, int h, int bd, const uint8_t *mi, int mi_rows, int mi_stride, void *ry, void *rcb, void *rcr, void *sy, void *scb,
            void *scr, int32_t *levels, int sharpness, int plane_start, int plane_end, int only_4x4, uint64_t *sse, int32_t *trace, int trace_cap,
            int32_t *n_trace)
{
    void *rp[3] = {ry, rcb, rcr}, *sp[3] = {sy, scb, scr};
    PictureControlSet_t *pcs = (PictureControlSet_t *)calloc(1, sizeof(*pcs));
    PictureParentControlSet_t *ppcs = (PictureParentControlSet_t *)calloc(1, sizeof(*ppcs));
    SequenceControlSet_t *scs = (SequenceControlSet_t *)calloc(1, sizeof(*scs));
    EbObjectWrapper_t *wrap = (EbObjectWrapper_t *)calloc(1, sizeof(*wrap));
    DlfContext_t *ctx = (DlfContext_t *)calloc(1, sizeof(*ctx));
    const size_t cells = (size_t)mi_rows * mi_stride;
    ModeInfo *cell = (ModeInfo *)calloc(cells, sizeof(*cell));
    ModeInfo **grid = (ModeInfo **)calloc(cells, sizeof(*grid));
    Pic recon, source, temp;

    if ((w + 63) / 64 * 16 != mi_stride) return -1;
    pic_init(&recon, w, h, bd, rp);
    pic_init(&source, w, h, bd, sy ? sp : NULL);
    pic_init(&temp, w, h, bd, NULL);
    for (size_t i = 0; i < cells; i++) {
        cell[i].mbmi.sb_type = (BlockSize)mi[4 * i];
        cell[i].mbmi.tx_size = (TxSize)mi[4 * i + 1];
        cell[i].mbmi.skip = mi[4 * i + 2] & 1;
        cell[i].mbmi.ref_frame[0] = (mi[4 * i + 2] & 1) ? LAST_FRAME : INTRA_FRAME;
        cell[i].mbmi.mode = DC_PRED;
        grid[i] = &cell[i];
    }
    scs->static_config.encoder_bit_depth = (uint32_t)bd;
    scs->sb_size = BLOCK_64X64;
    scs->sb_size_pix = 64;
    scs->luma_width = (uint16_t)w;
    scs->luma_height = (uint16_t)h;
    scs->chroma_width = (uint16_t)(w / 2);
    scs->chroma_height = (uint16_t)(h / 2);
    scs->picture_width_in_sb = (uint8_t)((w + 63) / 64);
    wrap->objectPtr = scs;
    ppcs->sequence_control_set_wrapper_ptr = wrap;
    ppcs->sequence_control_set_ptr = scs;
    ppcs->enhanced_picture_ptr = &source.d;
    ppcs->is_used_as_reference_flag = EB_FALSE;
    ppcs->tx_mode = only_4x4 ? ONLY_4X4 : TX_MODE_SELECT;
    ppcs->av1FrameType = KEY_FRAME;
    ppcs->lf.mode_ref_delta_enabled = 0;
    ppcs->lf.sharpness_level = sharpness;
    ppcs->lf.filter_level[0] = levels[0];
    ppcs->lf.filter_level[1] = levels[1];
    ppcs->lf.filter_level_u = levels[2];
    ppcs->lf.filter_level_v = levels[3];
    pcs->parent_pcs_ptr = ppcs;
    pcs->mi_grid_base = grid;
    pcs->recon_picture_ptr = pcs->recon_picture16bit_ptr = &recon.d;
    pcs->input_frame16bit = &source.d;
    ctx->temp_lf_recon_picture_ptr = ctx->temp_lf_recon_picture16bit_ptr = &temp.d;
    av1_loop_filter_init(pcs);

    G.pcs = pcs;
    G.trace = (int32_t(*)[4])trace;
    G.cap = trace_cap;
    G.n_trace = 0;
    if (op == 0 || op == 2) {
        av1_loop_filter_frame(&recon.d, pcs, plane_start, plane_end);
        if (op == 2) *sse = PictureSseCalculations(pcs, &recon.d, plane_start);
    } else {
        av1_pick_filter_level(ctx, &source.d, pcs, LPF_PICK_FROM_FULL_IMAGE);
        levels[0] = ppcs->lf.filter_level[0];
        levels[1] = ppcs->lf.filter_level[1];
        levels[2] = ppcs->lf.filter_level_u;
        levels[3] = ppcs->lf.filter_level_v;
    }
    if (n_trace) *n_trace = G.n_trace;
    G.pcs = NULL;
    G.trace = NULL;
    pic_out(&recon, w, h, bd, rp);
    pic_free(&recon); pic_free(&source); pic_free(&temp);
    free(grid); free(cell); free(ctx); free(wrap); free(scs); free(ppcs); free(pcs);
    return 0;
}
