/*
 * tests/golden/ref_lr_sgr_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own self-guided restoration search and frame filter for tests/golden/make_golden_lr_sgr.py.  Contains no
 * reference code: it is tests/golden/ref_lr_driver.c (which is the reference's EbRestorationPick.c included where it lies at build time,
 * plus the picture scaffolding drv_lr_open / drv_lr_units / drv_lr_close) followed by entry points that only call the reference's
 * functions and note what they return:
 *   drv_sgr_search   per unit of one plane and per parameter set: apply_sgr, the five sums of get_proj_subspace counted as integers on the
 *                    reference's flt0 / flt1, the dispatched get_proj_subspace, encode_xq and finer_search_pixel_proj_error; the trials of
 *                    the walk are noted by a shim behind the av1_[lowbd|highbd]_pixel_proj_error dispatch pointers (the decoded xq of each
 *                    call and the error it returned).  Then search_sgrproj_seg itself for the unit's SgrprojInfo and sse[RESTORE_SGRPROJ].
 *                    Also: the sum and the sum of squares of flt0 / flt1 per parameter set over the plane, and flt - u of chosen sets.
 *   drv_sgr_filter   av1_loop_restoration_filter_frame on a copy of the CDEF'd planes with frame types, unit types, taps and SgrprojInfo given
 *   drv_sgr_time     search_sgrproj_seg over all units of the three planes, timed (the CPU yardstick of tools/lr_sgr_probe.py)
 */
#include "ref_lr_driver.c"

#define SGR_TRACE_CAP 48

typedef struct {
    int64_t sums[5];
    int32_t exq[2], start_xqd[2], xqd[2];
    int64_t err;
    int32_t n_trials, reserved;
} SgrDetail;

static struct {
    int n_trace, on;
    int32_t trace_xq[SGR_TRACE_CAP][2];
    int64_t trace_err[SGR_TRACE_CAP];
    int64_t (*fwd8)(const uint8_t *, int32_t, int32_t, int32_t, const uint8_t *, int32_t, int32_t *, int32_t, int32_t *, int32_t, int32_t[2],
                    const sgr_params_type *);
    int64_t (*fwd16)(const uint8_t *, int32_t, int32_t, int32_t, const uint8_t *, int32_t, int32_t *, int32_t, int32_t *, int32_t, int32_t[2],
                     const sgr_params_type *);
    /* visitor outputs */
    SgrDetail *detail;
    int32_t *sgrproj, *trace_xq_out;
    int64_t *sse, *trace_err_out, *flt_sums;
    const int32_t *dump_ep;
    int32_t *dump;
    int32_t *flt;
} S;

static void sgr_note(const int32_t xq[2], int64_t err)
{
    if (!S.on) return;
    if (S.n_trace < SGR_TRACE_CAP) {
        S.trace_xq[S.n_trace][0] = xq[0], S.trace_xq[S.n_trace][1] = xq[1];
        S.trace_err[S.n_trace] = err;
    }
    S.n_trace++;
}

static int64_t sgr_shim8(const uint8_t *src8, int32_t w, int32_t h, int32_t ss, const uint8_t *dat8, int32_t ds, int32_t *f0, int32_t f0s, int32_t *f1,
                         int32_t f1s, int32_t xq[2], const sgr_params_type *params)
{
    const int64_t e = S.fwd8(src8, w, h, ss, dat8, ds, f0, f0s, f1, f1s, xq, params);
    sgr_note(xq, e);
    return e;
}

static int64_t sgr_shim16(const uint8_t *src8, int32_t w, int32_t h, int32_t ss, const uint8_t *dat8, int32_t ds, int32_t *f0, int32_t f0s, int32_t *f1,
                          int32_t f1s, int32_t xq[2], const sgr_params_type *params)
{
    const int64_t e = S.fwd16(src8, w, h, ss, dat8, ds, f0, f0s, f1, f1s, xq, params);
    sgr_note(xq, e);
    return e;
}

static int sample(const uint8_t *buf8, int stride, int y, int x)
{
    return G.hbd ? CONVERT_TO_SHORTPTR(buf8)[y * stride + x] : buf8[y * stride + x];
}

static void visit_sgr(const RestorationTileLimits *limits, const AV1PixelRect *tile_rect, int32_t idx, void *priv)
{
    RestSearchCtxt *rsc = (RestSearchCtxt *)priv;
    const int plane = rsc->plane, ss = plane > 0, pu = RESTORATION_PROC_UNIT_SIZE >> ss;
    const int w = limits->h_end - limits->h_start, h = limits->v_end - limits->v_start;
    uint8_t *dgd = rsc->dgd_buffer + limits->v_start * rsc->dgd_stride + limits->h_start;
    const uint8_t *src = rsc->src_buffer + limits->v_start * rsc->src_stride + limits->h_start;
    const int pw = G.w >> ss;
    int32_t *flt0 = S.flt, *flt1 = S.flt + RESTORATION_UNITPELS_MAX;
    const int fs = ((w + 7) & ~7) + 8;

    for (int ep = 0; ep < SGRPROJ_PARAMS; ep++) {
        const sgr_params_type *params = &sgr_params[ep];
        SgrDetail *d = &S.detail[idx * SGRPROJ_PARAMS + ep];
        int slot = -1;
        for (int k = 0; k < 3; k++)
            if (S.dump && S.dump_ep[k] == ep) slot = k;
        memset(d, 0, sizeof(*d));
        apply_sgr(ep, dgd, w, h, rsc->dgd_stride, G.hbd, G.bd, pu, pu, flt0, flt1, fs);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const int64_t u = (int64_t)sample(dgd, rsc->dgd_stride, y, x) << SGRPROJ_RST_BITS;
                const int64_t s = ((int64_t)sample(src, rsc->src_stride, y, x) << SGRPROJ_RST_BITS) - u;
                const int64_t a = params->r[0] > 0 ? flt0[y * fs + x] : u, b = params->r[1] > 0 ? flt1[y * fs + x] : u;
                const int64_t f0 = a - u, f1 = b - u;
                d->sums[0] += f0 * f0, d->sums[1] += f1 * f1, d->sums[2] += f0 * f1, d->sums[3] += f0 * s, d->sums[4] += f1 * s;
                if (params->r[0] > 0) S.flt_sums[ep * 4 + 0] += a, S.flt_sums[ep * 4 + 1] += a * a;
                if (params->r[1] > 0) S.flt_sums[ep * 4 + 2] += b, S.flt_sums[ep * 4 + 3] += b * b;
                if (slot >= 0) {
                    int32_t *o = S.dump + ((size_t)slot * 2 * (G.h >> ss) + (limits->v_start + y)) * pw + limits->h_start + x;
                    o[0] = (int32_t)f0;
                    o[(size_t)(G.h >> ss) * pw] = (int32_t)f1;
                }
            }
        get_proj_subspace(src, w, h, rsc->src_stride, dgd, rsc->dgd_stride, G.hbd, flt0, fs, flt1, fs, d->exq, params);
        encode_xq(d->exq, d->start_xqd, params);
        d->xqd[0] = d->start_xqd[0], d->xqd[1] = d->start_xqd[1];
        S.n_trace = 0, S.on = 1;
        d->err = finer_search_pixel_proj_error(src, w, h, rsc->src_stride, dgd, rsc->dgd_stride, G.hbd, flt0, fs, flt1, fs, 2, d->xqd, params);
        S.on = 0;
        d->n_trials = S.n_trace;
        const int nt = S.n_trace < SGR_TRACE_CAP ? S.n_trace : SGR_TRACE_CAP;
        memcpy(S.trace_xq_out + ((size_t)idx * SGRPROJ_PARAMS + ep) * SGR_TRACE_CAP * 2, S.trace_xq, sizeof(int32_t) * 2 * nt);
        memcpy(S.trace_err_out + ((size_t)idx * SGRPROJ_PARAMS + ep) * SGR_TRACE_CAP, S.trace_err, sizeof(int64_t) * nt);
    }
    search_sgrproj_seg(limits, tile_rect, idx, priv);
    S.sgrproj[4 * idx] = G.rusi[idx].sgrproj.ep;
    S.sgrproj[4 * idx + 1] = G.rusi[idx].sgrproj.xqd[0];
    S.sgrproj[4 * idx + 2] = G.rusi[idx].sgrproj.xqd[1];
    S.sgrproj[4 * idx + 3] = 0;
    S.sse[idx] = G.rusi[idx].sse[RESTORE_SGRPROJ];
}

static void sgr_hook(int on)
{
    if (on) {
        S.fwd8 = av1_lowbd_pixel_proj_error, S.fwd16 = av1_highbd_pixel_proj_error;
        av1_lowbd_pixel_proj_error = sgr_shim8, av1_highbd_pixel_proj_error = sgr_shim16;
    } else {
        av1_lowbd_pixel_proj_error = S.fwd8, av1_highbd_pixel_proj_error = S.fwd16;
    }
}

/* per unit of `plane`: detail[16] (80 bytes each), sgrproj[4] = ep, xqd0, xqd1, 0, sse = sse[RESTORE_SGRPROJ], trace_xq[16][CAP][2],
 * trace_err[16][CAP]; per plane flt_sums[16][4] = sum flt0, sum flt0^2, sum flt1, sum flt1^2; dump (may be null): [3][2][plane h][plane w]
 * flt0 - u, flt1 - u of the sets dump_ep[3].  Returns the trace cap. */
int drv_sgr_search(int plane, void *detail, int32_t *sgrproj, int64_t *sse, int32_t *trace_xq, int64_t *trace_err, int64_t *flt_sums,
                   const int32_t *dump_ep, int32_t *dump)
{
    const int n = G.cm.rst_info[plane].units_per_tile;
    S.detail = (SgrDetail *)detail, S.sgrproj = sgrproj, S.sse = sse, S.trace_xq_out = trace_xq, S.trace_err_out = trace_err;
    S.flt_sums = flt_sums, S.dump_ep = dump_ep, S.dump = dump;
    S.flt = (int32_t *)calloc(2 * RESTORATION_UNITPELS_MAX, sizeof(int32_t));
    memset(flt_sums, 0, sizeof(int64_t) * SGRPROJ_PARAMS * 4);
    G.rusi = (RestUnitSearchInfo *)calloc(n, sizeof(RestUnitSearchInfo));
    rsc_setup(plane);
    sgr_hook(1);
    av1_foreach_rest_unit_in_frame(&G.cm, plane, rsc_on_tile, visit_sgr, &G.rsc);
    sgr_hook(0);
    free(G.rusi);
    free(S.flt);
    return SGR_TRACE_CAP;
}

/* as drv_lr_filter, with unit_sgr[unit][4] = ep, xqd0, xqd1, 0 for the RESTORE_SGRPROJ units */
int drv_sgr_filter(const int32_t frame_type[3], const int32_t unit_base[3], const uint8_t *unit_type, const int16_t *unit_taps, const int32_t *unit_sgr,
                   void *const out[3])
{
    Pic frame;
    pic_init(&frame, G.w, G.h, G.hbd, NULL);
    pic_copy(&frame, &G.cdef, G.w, G.h, G.hbd);
    for (int p = 0; p < 3; p++) {
        RestorationInfo *rsi = &G.cm.rst_info[p];
        rsi->frame_restoration_type = (RestorationType)frame_type[p];
        for (int i = 0; i < rsi->units_per_tile; i++) {
            const int u = unit_base[p] + i;
            memset(&rsi->unit_info[i], 0, sizeof(rsi->unit_info[i]));
            rsi->unit_info[i].restoration_type = (RestorationType)unit_type[u];
            memcpy(rsi->unit_info[i].wiener_info.vfilter, unit_taps + 16 * u, 16);
            memcpy(rsi->unit_info[i].wiener_info.hfilter, unit_taps + 16 * u + 8, 16);
            rsi->unit_info[i].sgrproj_info.ep = unit_sgr[4 * u];
            rsi->unit_info[i].sgrproj_info.xqd[0] = unit_sgr[4 * u + 1];
            rsi->unit_info[i].sgrproj_info.xqd[1] = unit_sgr[4 * u + 2];
        }
    }
    G.cm.rst_tmpbuf = G.tmpbuf;
    memset(&G.cm.rst_frame, 0, sizeof(G.cm.rst_frame));
    av1_loop_restoration_filter_frame(&frame.y, &G.cm, 0);
    pic_out(&frame, G.w, G.h, G.hbd, out);
    pic_free(&frame);
    return 0;
}

static void visit_sgr_time(const RestorationTileLimits *limits, const AV1PixelRect *tile_rect, int32_t idx, void *priv)
{
    search_sgrproj_seg(limits, tile_rect, idx, priv);
}

/* seconds of search_sgrproj_seg over all units of the three planes, one thread */
double drv_sgr_time(void)
{
    struct timespec a, b;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int plane = 0; plane < 3; plane++) {
        G.rusi = (RestUnitSearchInfo *)calloc(G.cm.rst_info[plane].units_per_tile, sizeof(RestUnitSearchInfo));
        rsc_setup(plane);
        av1_foreach_rest_unit_in_frame(&G.cm, plane, rsc_on_tile, visit_sgr_time, &G.rsc);
        free(G.rusi);
    }
    clock_gettime(CLOCK_MONOTONIC, &b);
    return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec);
}
