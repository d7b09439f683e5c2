/*
 * tests/golden/ref_lr_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own Wiener loop-restoration search and frame filter for tests/golden/make_golden_lr.py.  Contains no reference
 * code: search_norestore_seg, search_wiener_seg, try_restoration_unit_seg, wiener_decompose_sep_sym, finalize_sym_filter and
 * compute_score are `static`, so this translation unit is the reference's EbRestorationPick.c itself, included where it lies at build
 * time (nothing of it is copied into the repository; make_golden_lr.py links this file INSTEAD of EbRestorationPick.o), followed by
 * entry points that only fill the structures those functions read (an Av1Common with its RestorationInfo and stripe-boundary buffers
 * from av1_alloc_restoration_buffers, Yv12BufferConfig descriptors over bordered copies of the caller's planes) and call them:
 *   drv_lr_open     the three sets of planes; av1_loop_restoration_save_boundary_lines on the deblocked planes (after_cdef 0) and on the
 *                   CDEF'd ones (after_cdef 1), as EbCdefProcess.c:498,576 does, and extend_frame on the CDEF'd planes
 *   drv_lr_units    av1_foreach_rest_unit_in_frame with a visitor that notes each unit's limits
 *   drv_lr_search   per unit of one plane: the dispatched av1_compute_stats[_highbd] and find_average[_highbd], the solve
 *                   (wiener_decompose_sep_sym, finalize_sym_filter twice, compute_score), then search_norestore_seg and
 *                   search_wiener_seg themselves.  The order of trial filters is noted by a shim behind the av1_[highbd_]wiener_convolve_
 *                   add_src dispatch pointers: it notes the taps of the call that writes the unit's first sample and forwards every call.
 *                   Each noted trial is then run again through try_restoration_unit_seg for its SSE.
 *   drv_lr_filter   av1_loop_restoration_filter_frame on a copy of the CDEF'd planes with the frame and unit types and taps given
 *   drv_lr_time     search_norestore_seg + search_wiener_seg over all planes, timed (the CPU yardstick of tools/lr_probe.py)
 */
#define RTCD_C
#include "EbRestorationPick.c"

#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "aom_dsp_rtcd.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;
void av1_loop_restoration_save_boundary_lines(const Yv12BufferConfig *frame, Av1Common *cm, int32_t after_cdef);

#define MARGIN 32
#define TRACE_CAP 128

/* The 10-bit SSE goes through aom_highbd_8_mse16x16_sse2 (ASM_SSE2/highbd_variance_sse2.c:195), whose 16x16 leaf is NASM code the link
 * does not have.  Stand-in with the leaf's contract: sum and sum of squares of the differences of one 16x16 block. */
uint32_t aom_highbd_calc16x16var_sse2(const uint16_t *src, int32_t src_stride, const uint16_t *ref, int32_t ref_stride, uint32_t *sse, int32_t *sum)
{
    uint32_t q = 0;
    int32_t s = 0;
    for (int y = 0; y < 16; y++)
        for (int x = 0; x < 16; x++) {
            const int32_t d = (int32_t)src[y * src_stride + x] - (int32_t)ref[y * ref_stride + x];
            s += d;
            q += (uint32_t)(d * d);
        }
    *sse = q;
    *sum = s;
    return 0;
}

/* aom_clear_system_state is RunEmms, NASM code as well: it only resets the x87 / MMX state, which nothing here uses. */
void RunEmms(void) {}

typedef struct {
    Yv12BufferConfig y;
    uint8_t *mem[3];
} Pic;

static struct {
    Av1Common cm;
    PictureParentControlSet_t *ppcs;
    Pic cdef, dbk, src, trial;
    int w, h, bd, hbd;
    int32_t *tmpbuf;
    /* the shim's notes */
    uint8_t *unit_dst;
    int n_trace;
    int16_t trace[TRACE_CAP][16];
    void (*fwd8)(const uint8_t *, ptrdiff_t, uint8_t *, ptrdiff_t, const int16_t *, int32_t, const int16_t *, int32_t, int32_t, int32_t,
                 const ConvolveParams *);
    void (*fwd16)(const uint8_t *, ptrdiff_t, uint8_t *, ptrdiff_t, const int16_t *, int32_t, const int16_t *, int32_t, int32_t, int32_t,
                  const ConvolveParams *, int32_t);
    /* visitor outputs */
    int32_t *limits;
    int n_units;
    int64_t *M, *H, *sse, *trace_sse;
    int32_t *avg, *rejected, *n_trials;
    int16_t *start, *final_taps, *trace_taps;
    RestUnitSearchInfo *rusi;
    RestSearchCtxt rsc;
} G;

static void note(uint8_t *dst, const int16_t *fx, const int16_t *fy)
{
    if (dst != G.unit_dst) return;
    if (G.n_trace < TRACE_CAP) {
        memcpy(G.trace[G.n_trace], fy, 16);
        memcpy(G.trace[G.n_trace] + 8, fx, 16);
    }
    G.n_trace++;
}

static void shim8(const uint8_t *src, ptrdiff_t ss, uint8_t *dst, ptrdiff_t ds, const int16_t *fx, int32_t xs, const int16_t *fy, int32_t ys,
                  int32_t w, int32_t h, const ConvolveParams *cp)
{
    note(dst, fx, fy);
    G.fwd8(src, ss, dst, ds, fx, xs, fy, ys, w, h, cp);
}

static void shim16(const uint8_t *src, ptrdiff_t ss, uint8_t *dst, ptrdiff_t ds, const int16_t *fx, int32_t xs, const int16_t *fy, int32_t ys,
                   int32_t w, int32_t h, const ConvolveParams *cp, int32_t bd)
{
    note(dst, fx, fy);
    G.fwd16(src, ss, dst, ds, fx, xs, fy, ys, w, h, cp, bd);
}

static void pic_init(Pic *p, int w, int h, int hbd, void *const planes[3])
{
    const int b = hbd ? 2 : 1;
    memset(p, 0, sizeof(*p));
    for (int i = 0; i < 3; i++) {
        const int pw = i ? w / 2 : w, ph = i ? h / 2 : h, s = pw + 2 * MARGIN;
        p->mem[i] = (uint8_t *)calloc((size_t)s * (ph + 2 * MARGIN) + 64, b);
        uint8_t *origin = p->mem[i] + ((size_t)MARGIN * s + MARGIN) * b;
        if (planes)
            for (int y = 0; y < ph; y++) memcpy(origin + (size_t)y * s * b, (const uint8_t *)planes[i] + (size_t)y * pw * b, (size_t)pw * b);
        p->y.buffers[i] = hbd ? CONVERT_TO_BYTEPTR(origin) : origin;
        p->y.strides[i] = s;
        p->y.widths[i] = pw;
        p->y.heights[i] = ph;
        if (i < 2) {
            p->y.crop_widths[i] = pw;
            p->y.crop_heights[i] = ph;
        }
    }
    p->y.subsampling_x = p->y.subsampling_y = 1;
    p->y.border = MARGIN;
    p->y.flags = hbd ? YV12_FLAG_HIGHBITDEPTH : 0;
}

static void pic_copy(Pic *d, const Pic *s, int w, int h, int hbd)
{
    for (int i = 0; i < 3; i++) {
        const int pw = i ? w / 2 : w, ph = i ? h / 2 : h;
        memcpy(d->mem[i], s->mem[i], ((size_t)(pw + 2 * MARGIN) * (ph + 2 * MARGIN) + 64) * (hbd ? 2 : 1));
    }
}

static void pic_out(const Pic *p, int w, int h, int hbd, void *const planes[3])
{
    const int b = hbd ? 2 : 1;
    for (int i = 0; i < 3; i++) {
        const int pw = i ? w / 2 : w, ph = i ? h / 2 : h, s = pw + 2 * MARGIN;
        const uint8_t *origin = p->mem[i] + ((size_t)MARGIN * s + MARGIN) * b;
        for (int y = 0; y < ph; y++) memcpy((uint8_t *)planes[i] + (size_t)y * pw * b, origin + (size_t)y * s * b, (size_t)pw * b);
    }
}

static void pic_free(Pic *p)
{
    for (int i = 0; i < 3; i++) free(p->mem[i]);
}

int drv_lr_open(int w, int h, int bd, const int32_t unit_size[3], void *const cdef[3], void *const dbk[3], void *const src[3])
{
    static EbMemoryMapEntry *mm = NULL;
    static uint32_t mm_index;
    static uint64_t mm_total;
    if (!mm) mm = (EbMemoryMapEntry *)calloc(1 << 16, sizeof(EbMemoryMapEntry));
    memoryMap = mm;
    mm_index = 0;
    memoryMapIndex = &mm_index;
    totalLibMemory = &mm_total;
    setup_rtcd_internal(ASM_AVX2);
    G.fwd8 = av1_wiener_convolve_add_src;
    G.fwd16 = av1_highbd_wiener_convolve_add_src;
    av1_wiener_convolve_add_src = shim8;
    av1_highbd_wiener_convolve_add_src = shim16;

    G.w = w, G.h = h, G.bd = bd, G.hbd = bd > 8;
    memset(&G.cm, 0, sizeof(G.cm));
    G.ppcs = (PictureParentControlSet_t *)calloc(1, sizeof(*G.ppcs));
    G.cm.p_pcs_ptr = G.ppcs;
    G.cm.mi_rows = h / 4;
    G.cm.mi_cols = w / 4;
    G.cm.use_highbitdepth = G.hbd;
    G.cm.bit_depth = bd;
    G.cm.subsampling_x = G.cm.subsampling_y = 1;
    G.cm.width = G.cm.superres_upscaled_width = w;
    G.cm.height = G.cm.superres_upscaled_height = h;
    for (int p = 0; p < 3; p++) G.cm.rst_info[p].restoration_unit_size = unit_size[p];
    if (av1_alloc_restoration_buffers(&G.cm) != EB_ErrorNone) return -1;
    pic_init(&G.cdef, w, h, G.hbd, cdef);
    pic_init(&G.dbk, w, h, G.hbd, dbk);
    pic_init(&G.src, w, h, G.hbd, src);
    pic_init(&G.trial, w, h, G.hbd, NULL);
    G.cm.frame_to_show = &G.cdef.y;
    G.tmpbuf = (int32_t *)calloc(1, RESTORATION_TMPBUF_SIZE);
    av1_loop_restoration_save_boundary_lines(&G.dbk.y, &G.cm, 0);
    av1_loop_restoration_save_boundary_lines(&G.cdef.y, &G.cm, 1);
    for (int p = 0; p < 3; p++)
        extend_frame(G.cdef.y.buffers[p], G.cdef.y.crop_widths[p > 0], G.cdef.y.crop_heights[p > 0], G.cdef.y.strides[p > 0], RESTORATION_BORDER,
                     RESTORATION_BORDER, G.hbd);
    return 0;
}

void drv_lr_close(void)
{
    av1_wiener_convolve_add_src = G.fwd8;
    av1_highbd_wiener_convolve_add_src = G.fwd16;
    pic_free(&G.cdef), pic_free(&G.dbk), pic_free(&G.src), pic_free(&G.trial);
    free(G.tmpbuf);
    free(G.ppcs);
}

static void visit_limits(const RestorationTileLimits *limits, const AV1PixelRect *tile_rect, int32_t idx, void *priv)
{
    (void)tile_rect, (void)priv;
    int32_t *o = G.limits + 4 * idx;
    o[0] = limits->h_start, o[1] = limits->h_end, o[2] = limits->v_start, o[3] = limits->v_end;
    if (idx + 1 > G.n_units) G.n_units = idx + 1;
}

/* limits[n][4] = h_start, h_end, v_start, v_end; returns the number of units, horz_units_per_tile in *horz */
int drv_lr_units(int plane, int32_t *limits, int32_t *horz)
{
    G.limits = limits;
    G.n_units = 0;
    av1_foreach_rest_unit_in_frame(&G.cm, plane, NULL, visit_limits, NULL);
    *horz = G.cm.rst_info[plane].horz_units_per_tile;
    return G.n_units;
}

static void visit_search(const RestorationTileLimits *limits, const AV1PixelRect *tile_rect, int32_t idx, void *priv)
{
    RestSearchCtxt *rsc = (RestSearchCtxt *)priv;
    const int plane = rsc->plane, win = plane ? WIENER_WIN_CHROMA : WIENER_WIN, n = win * win;
    int64_t M[WIENER_WIN2], H[WIENER_WIN2 * WIENER_WIN2];
    int32_t vd[WIENER_WIN], hd[WIENER_WIN];
    RestorationUnitInfo rui;

    if (G.hbd) {
        av1_compute_stats_highbd(win, rsc->dgd_buffer, rsc->src_buffer, limits->h_start, limits->h_end, limits->v_start, limits->v_end,
                                 rsc->dgd_stride, rsc->src_stride, M, H, (aom_bit_depth_t)G.bd);
        G.avg[idx] = find_average_highbd(CONVERT_TO_SHORTPTR(rsc->dgd_buffer), limits->h_start, limits->h_end, limits->v_start, limits->v_end,
                                         rsc->dgd_stride);
    } else {
        av1_compute_stats(win, rsc->dgd_buffer, rsc->src_buffer, limits->h_start, limits->h_end, limits->v_start, limits->v_end, rsc->dgd_stride,
                          rsc->src_stride, M, H);
        G.avg[idx] = find_average(rsc->dgd_buffer, limits->h_start, limits->h_end, limits->v_start, limits->v_end, rsc->dgd_stride);
    }
    memcpy(G.M + (size_t)idx * WIENER_WIN2, M, sizeof(int64_t) * n);
    memcpy(G.H + (size_t)idx * WIENER_WIN2 * WIENER_WIN2, H, sizeof(int64_t) * n * n);
    /* the solve consumes M and H: on copies */
    memset(&rui, 0, sizeof(rui));
    wiener_decompose_sep_sym(win, M, H, vd, hd);
    finalize_sym_filter(win, vd, rui.wiener_info.vfilter);
    finalize_sym_filter(win, hd, rui.wiener_info.hfilter);
    memcpy(G.start + 16 * idx, rui.wiener_info.vfilter, 16);
    memcpy(G.start + 16 * idx + 8, rui.wiener_info.hfilter, 16);
    G.rejected[idx] = compute_score(win, M, H, rui.wiener_info.vfilter, rui.wiener_info.hfilter) > 0;

    /* the search itself */
    const int is_uv = plane > 0;
    uint8_t *dst = rsc->dst->buffers[plane] + limits->v_start * rsc->dst->strides[is_uv] + limits->h_start;
    G.unit_dst = dst;
    G.n_trace = 0;
    search_norestore_seg(limits, tile_rect, idx, priv);
    search_wiener_seg(limits, tile_rect, idx, priv);
    G.unit_dst = NULL;
    G.sse[2 * idx] = G.rusi[idx].sse[RESTORE_NONE];
    G.sse[2 * idx + 1] = G.rusi[idx].sse[RESTORE_WIENER];
    memcpy(G.final_taps + 16 * idx, G.rusi[idx].wiener.vfilter, 16);
    memcpy(G.final_taps + 16 * idx + 8, G.rusi[idx].wiener.hfilter, 16);
    G.n_trials[idx] = G.n_trace;
    const int nt = G.n_trace < TRACE_CAP ? G.n_trace : TRACE_CAP;
    memcpy(G.trace_taps + (size_t)idx * TRACE_CAP * 16, G.trace, sizeof(int16_t) * 16 * nt);
    for (int t = 0; t < nt; t++) {
        memset(&rui, 0, sizeof(rui));
        rui.restoration_type = RESTORE_WIENER;
        memcpy(rui.wiener_info.vfilter, G.trace[t], 16);
        memcpy(rui.wiener_info.hfilter, G.trace[t] + 8, 16);
        G.trace_sse[(size_t)idx * TRACE_CAP + t] = try_restoration_unit_seg(rsc, limits, tile_rect, &rui);
    }
}

static void rsc_setup(int plane)
{
    memset(&G.rsc, 0, sizeof(G.rsc));
    init_rsc_seg(&G.cdef.y, &G.src.y, &G.cm, NULL, plane, G.rusi, &G.trial.y, &G.rsc);
    G.rsc.tmpbuf = G.tmpbuf;
}

/* per unit of `plane`: M[49], H[49*49] (the first win^2 resp. win^4 entries used), avg, rejected, start[16] = vfilter, hfilter,
 * sse[2] = RESTORE_NONE, RESTORE_WIENER, final[16], n_trials, trace_taps[TRACE_CAP][16], trace_sse[TRACE_CAP] */
int drv_lr_search(int plane, int64_t *M, int64_t *H, int32_t *avg, int32_t *rejected, int16_t *start, int64_t *sse, int16_t *final_taps,
                  int32_t *n_trials, int16_t *trace_taps, int64_t *trace_sse)
{
    const int n = G.cm.rst_info[plane].units_per_tile;
    G.M = M, G.H = H, G.avg = avg, G.rejected = rejected, G.start = start, G.sse = sse, G.final_taps = final_taps, G.n_trials = n_trials;
    G.trace_taps = trace_taps, G.trace_sse = trace_sse;
    G.rusi = (RestUnitSearchInfo *)calloc(n, sizeof(RestUnitSearchInfo));
    rsc_setup(plane);
    av1_foreach_rest_unit_in_frame(&G.cm, plane, rsc_on_tile, visit_search, &G.rsc);
    free(G.rusi);
    return TRACE_CAP;
}

/* frame_type[3], unit_type / unit_taps: per plane at unit_base[p] the units of that plane (taps: vfilter[8], hfilter[8]) */
int drv_lr_filter(const int32_t frame_type[3], const int32_t unit_base[3], const uint8_t *unit_type, const int16_t *unit_taps, void *const out[3])
{
    Pic frame;
    pic_init(&frame, G.w, G.h, G.hbd, NULL);
    pic_copy(&frame, &G.cdef, G.w, G.h, G.hbd);
    for (int p = 0; p < 3; p++) {
        RestorationInfo *rsi = &G.cm.rst_info[p];
        rsi->frame_restoration_type = (RestorationType)frame_type[p];
        for (int i = 0; i < rsi->units_per_tile; i++) {
            memset(&rsi->unit_info[i], 0, sizeof(rsi->unit_info[i]));
            rsi->unit_info[i].restoration_type = (RestorationType)unit_type[unit_base[p] + i];
            memcpy(rsi->unit_info[i].wiener_info.vfilter, unit_taps + 16 * (unit_base[p] + i), 16);
            memcpy(rsi->unit_info[i].wiener_info.hfilter, unit_taps + 16 * (unit_base[p] + i) + 8, 16);
        }
    }
    G.cm.rst_tmpbuf = G.tmpbuf;
    memset(&G.cm.rst_frame, 0, sizeof(G.cm.rst_frame));
    av1_loop_restoration_filter_frame(&frame.y, &G.cm, 0);
    pic_out(&frame, G.w, G.h, G.hbd, out);
    pic_free(&frame);
    return 0;
}

static void visit_time(const RestorationTileLimits *limits, const AV1PixelRect *tile_rect, int32_t idx, void *priv)
{
    search_norestore_seg(limits, tile_rect, idx, priv);
    search_wiener_seg(limits, tile_rect, idx, priv);
}

/* seconds of search_norestore_seg + search_wiener_seg over all units of the three planes; the number of trial filters in *trials */
double drv_lr_time(int64_t *trials)
{
    struct timespec a, b;
    G.unit_dst = NULL;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int plane = 0; plane < 3; plane++) {
        G.rusi = (RestUnitSearchInfo *)calloc(G.cm.rst_info[plane].units_per_tile, sizeof(RestUnitSearchInfo));
        rsc_setup(plane);
        av1_foreach_rest_unit_in_frame(&G.cm, plane, rsc_on_tile, visit_time, &G.rsc);
        free(G.rusi);
    }
    clock_gettime(CLOCK_MONOTONIC, &b);
    if (trials) *trials = 0;
    return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec);
}
