// svt-av1-1_amd/csrc/lr_abi.hip -- C-ABI glue of loop restoration: the exported entries that launch through
// lr_launch.h, with their validators and shared bodies.  Host code only.
#include "svthip_glue.h"
#include "lr_launch.h"

namespace {

// The restoration entries: one check of the picture for all of them.  Only the planes [plane_start, plane_end) are looked at; the source
// planes only where the entry compares against them.
int32_t check_lr_args(const svthip_lr_picture* pic, int bd, bool need_source, uint32_t plane_start, uint32_t plane_end)
{
    TRY(check_non_null({pic}));
    TRY(check_filter_bit_depth(bd));
    if (plane_start >= plane_end || plane_end > 3)
        return fail(SVTHIP_ERR_BAD_PARAMETER, "planes [%u, %u) are empty or not within 0..3", (unsigned)plane_start, (unsigned)plane_end);
    TRY(check_filter_picture_size(pic->width, pic->height));
    for (uint32_t p = 0; p < 3; p++)   // the unit index space spans all three planes
        if (pic->unit_size[p] != 64 && pic->unit_size[p] != 128 && pic->unit_size[p] != 256)
            return fail(SVTHIP_ERR_BAD_PARAMETER, "unit size of plane %d must be 64, 128 or 256 (got %u)", (int)p, (unsigned)pic->unit_size[p]);
    for (uint32_t p = plane_start; p < plane_end; p++) {
        const FilterPlane planes[3] = {{pic->cdef[p], pic->cdef_stride[p]}, {pic->deblocked[p], pic->deblocked_stride[p]},
                                       {pic->source[p], pic->source_stride[p]}};
        TRY(check_filter_planes(p, p ? pic->width / 2 : pic->width, bd, planes, need_source ? 3 : 2));
    }
    return SVTHIP_OK;
}

// the planes [ps, pe) the frame filter writes
int32_t check_lr_out_planes(const svthip_lr_picture* pic, void* const d_out[3], const uint32_t out_stride[3], uint32_t ps, uint32_t pe, int bd)
{
    for (uint32_t p = ps; p < pe; p++) {
        TRY(check_non_null({d_out[p]}));
        if (out_stride[p] < (p ? pic->width / 2 : pic->width))
            return fail(SVTHIP_ERR_BAD_PARAMETER, "output stride of plane %d is smaller than its width", (int)p);
        if (bd > 8 && !aligned(d_out[p], 2)) return fail(SVTHIP_ERR_BAD_PARAMETER, "16-bit planes must be 2-byte aligned");
    }
    return SVTHIP_OK;
}

int32_t check_lr_units(uint32_t unit_begin, uint32_t unit_end, uint32_t win)
{
    if (win != 5 && win != 7) return fail(SVTHIP_ERR_BAD_PARAMETER, "wiener_win must be 5 or 7 (got %u)", (unsigned)win);
    if (unit_begin > unit_end) return fail(SVTHIP_ERR_BAD_PARAMETER, "units [%u, %u) run backwards", (unsigned)unit_begin, (unsigned)unit_end);
    return SVTHIP_OK;
}

int32_t lr_stats_entry(svthip_ctx* ctx, const svthip_lr_picture* pic, uint32_t ps, uint32_t pe, int bd, int64_t* d_M, int64_t* d_H, int32_t* d_avg,
                       int64_t* d_sse_none, void* d_work, void* stream)
{
    TRY(check_lr_args(pic, bd, true, ps, pe));
    TRY(check_non_null({d_M, d_H, d_avg, d_sse_none, d_work}));
    if (!aligned({d_M, d_H, d_sse_none, d_work}, 8) || !aligned(d_avg, 4))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "d_M, d_H, d_sse_none and d_work must be 8-byte aligned, d_avg 4-byte");
    HIP_TRY(svthip::launch_lr_stats(*pic, (int)ps, (int)pe, bd, d_work, d_M, d_H, d_avg, d_sse_none, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t lr_trial_entry(svthip_ctx* ctx, const svthip_lr_picture* pic, uint32_t ps, uint32_t pe, int bd, const int16_t* d_taps, const uint8_t* d_skip,
                       int64_t* d_sse, void* stream)
{
    TRY(check_lr_args(pic, bd, true, ps, pe));
    TRY(check_non_null({d_taps, d_sse}));
    if (!aligned(d_taps, 2) || !aligned(d_sse, 8)) return fail(SVTHIP_ERR_BAD_PARAMETER, "d_taps must be 2-byte and d_sse 8-byte aligned");
    HIP_TRY(svthip::launch_lr_trial(*pic, (int)ps, (int)pe, bd, d_taps, 32, d_skip, 1, d_sse, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t lr_search_entry(svthip_ctx* ctx, const svthip_lr_picture* pic, uint32_t ps, uint32_t pe, int bd, uint32_t n_steps, uint32_t resume,
                        void* d_work, int64_t* d_sse, int16_t* d_taps, int32_t* d_n_trials, int32_t* d_pending, void* stream)
{
    TRY(check_lr_args(pic, bd, true, ps, pe));
    TRY(check_non_null({d_work, d_sse, d_taps, d_n_trials, d_pending}));
    if (!aligned({d_work, d_sse}, 8) || !aligned({d_n_trials, d_pending}, 4) || !aligned(d_taps, 2))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "d_work and d_sse must be 8-byte, d_n_trials and d_pending 4-byte, d_taps 2-byte aligned");
    HIP_TRY(svthip::launch_lr_search(*pic, (int)ps, (int)pe, bd, n_steps, resume != 0, d_work, d_sse, d_taps, d_n_trials, d_pending, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

// all_types: the entry for the three unit types, where d_taps and d_sgrproj may each be null (a unit that needs the missing one is refused
// on the device); otherwise the Wiener-only entry, which has no d_sgrproj and needs d_taps
int32_t lr_filter_frame_entry(svthip_ctx* ctx, const svthip_lr_picture* pic, void* const d_out[3], const uint32_t out_stride[3], uint32_t ps,
                              uint32_t pe, int bd, const uint8_t* d_unit_type, const int16_t* d_taps, const int32_t* d_sgrproj, bool all_types,
                              void* stream)
{
    TRY(check_lr_args(pic, bd, false, ps, pe));
    TRY(check_non_null({d_out, out_stride, d_unit_type}));
    if (!all_types) TRY(check_non_null({d_taps}));
    if (!aligned(d_taps, 2) || !aligned(d_sgrproj, 4)) return fail(SVTHIP_ERR_BAD_PARAMETER, "d_taps must be 2-byte and d_sgrproj 4-byte aligned");
    TRY(check_lr_out_planes(pic, d_out, out_stride, ps, pe, bd));
    hipStream_t s;
    uint32_t* d_refused;
    TRY(refused_counter(ctx, stream, &s, &d_refused));
    HIP_TRY(svthip::launch_lr_filter_frame(*pic, d_out, out_stride, (int)ps, (int)pe, bd, d_unit_type, d_taps, d_sgrproj, d_refused, s));
    return SVTHIP_OK;
}

// the self-guided entries: the picture through check_lr_args like the Wiener entries
int32_t sgr_plane_entry(svthip_ctx* ctx, const svthip_lr_picture* pic, uint32_t plane, int bd, uint32_t ep, int32_t* d_flt0, int32_t* d_flt1,
                        uint32_t flt_stride, void* stream)
{
    if (plane > 2) return fail(SVTHIP_ERR_BAD_PARAMETER, "plane must be 0..2 (got %u)", (unsigned)plane);
    TRY(check_lr_args(pic, bd, false, plane, plane + 1));
    if (ep > 15) return fail(SVTHIP_ERR_BAD_PARAMETER, "ep must be 0..15 (got %u)", (unsigned)ep);
    const bool r0 = !(ep >= 10 && ep < 14), r1 = ep < 14;
    if (r0) TRY(check_non_null({d_flt0}));
    if (r1) TRY(check_non_null({d_flt1}));
    if (!aligned({d_flt0, d_flt1}, 4)) return fail(SVTHIP_ERR_BAD_PARAMETER, "d_flt0 and d_flt1 must be 4-byte aligned");
    if (flt_stride < (plane ? pic->width / 2 : pic->width)) return fail(SVTHIP_ERR_BAD_PARAMETER, "flt_stride is smaller than the width of plane %u", (unsigned)plane);
    HIP_TRY(svthip::launch_sgr_plane(*pic, (int)plane, bd, (int)ep, d_flt0, d_flt1, flt_stride, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t sgr_search_entry(svthip_ctx* ctx, const svthip_lr_picture* pic, uint32_t ps, uint32_t pe, int bd, void* d_work, int32_t* d_sgrproj, int64_t* d_sse,
                         svthip_sgrproj_detail* d_detail, void* stream)
{
    TRY(check_lr_args(pic, bd, true, ps, pe));
    TRY(check_non_null({d_work, d_sgrproj, d_sse}));
    if (!aligned({d_work, d_sse, d_detail}, 8) || !aligned(d_sgrproj, 4))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "d_work, d_sse and d_detail must be 8-byte, d_sgrproj 4-byte aligned");
    HIP_TRY(svthip::launch_sgr_search(*pic, (int)ps, (int)pe, bd, d_work, d_sgrproj, d_sse, d_detail, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t sgr_trial_entry(svthip_ctx* ctx, const svthip_lr_picture* pic, uint32_t ps, uint32_t pe, int bd, const int32_t* d_sgrproj, const uint8_t* d_skip,
                        int64_t* d_sse, void* stream)
{
    TRY(check_lr_args(pic, bd, true, ps, pe));
    TRY(check_non_null({d_sgrproj, d_sse}));
    if (!aligned(d_sgrproj, 4) || !aligned(d_sse, 8)) return fail(SVTHIP_ERR_BAD_PARAMETER, "d_sgrproj must be 4-byte and d_sse 8-byte aligned");
    HIP_TRY(svthip::launch_sgr_trial(*pic, (int)ps, (int)pe, bd, d_sgrproj, d_skip, d_sse, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

// the decision's rate tables, host memory: nothing negative
int32_t check_rest_finish_rates(const svthip_rest_finish_rates* r)
{
    TRY(check_non_null({r}));
    const int32_t v[8] = {r->rdmult, r->wiener_cost[0], r->wiener_cost[1], r->sgrproj_cost[0], r->sgrproj_cost[1], r->switchable_cost[0],
                          r->switchable_cost[1], r->switchable_cost[2]};
    for (int i = 0; i < 8; i++)
        if (v[i] < 0) return fail(SVTHIP_ERR_BAD_PARAMETER, i ? "a restoration cost is negative (%d)" : "rdmult is negative (%d)", (int)v[i]);
    return SVTHIP_OK;
}

int32_t lr_pick_filter_entry(svthip_ctx* ctx, const svthip_lr_picture* pic, int bd, const svthip_rest_finish_rates* rates, void* d_work,
                             void* const d_out[3], const uint32_t out_stride[3], uint8_t* d_unit_type, int16_t* d_taps, int32_t* d_sgrproj,
                             svthip_rest_finish_result* d_result, void* stream)
{
    TRY(check_lr_args(pic, bd, true, 0, 3));
    TRY(check_rest_finish_rates(rates));
    TRY(check_non_null({d_work, d_out, out_stride, d_unit_type, d_taps, d_sgrproj, d_result}));
    if (!aligned({d_work, d_result}, 8) || !aligned(d_sgrproj, 4) || !aligned(d_taps, 2))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "d_work and d_result must be 8-byte, d_sgrproj 4-byte, d_taps 2-byte aligned");
    TRY(check_lr_out_planes(pic, d_out, out_stride, 0, 3, bd));
    hipStream_t s;
    uint32_t* d_refused;
    TRY(refused_counter(ctx, stream, &s, &d_refused));
    HIP_TRY(svthip::launch_lr_pick_filter(*pic, bd, *rates, d_work, d_out, out_stride, d_unit_type, d_taps, d_sgrproj, d_result, d_refused, s));
    return SVTHIP_OK;
}

}  // namespace

extern "C" {

// Wiener loop restoration (Codec/EbRestorationPick.c:743-1104, :1257-1366, :1742-1896; EbRestoration.c:1172-1341): statistics, solve, SSE
// trial, walk, the whole search, and the frame filter for RESTORE_NONE / RESTORE_WIENER units
uint32_t svthip_lr_unit_geometry(uint32_t width, uint32_t height, const uint32_t unit_size[3], uint32_t unit_base[4], int32_t* limits)
{
    uint32_t local[4];
    if (!unit_base) unit_base = local;
    for (int p = 0; p < 4; p++) unit_base[p] = 0;
    if (!unit_size || width == 0 || height == 0 || (width | height) % 8 != 0 || width > 16384 || height > 16384) return 0;
    for (int p = 0; p < 3; p++)
        if (unit_size[p] != 64 && unit_size[p] != 128 && unit_size[p] != 256) return 0;
    return svthip::lr_unit_geometry(width, height, unit_size, unit_base, limits);
}

size_t svthip_lr_workspace_bytes(uint32_t n_units) { return svthip::lr_workspace(n_units).total; }

uint32_t svthip_wiener_walk_max_trials(uint32_t wiener_win) { return wiener_win == 5 || wiener_win == 7 ? svthip::lr_walk_max_trials((int)wiener_win) : 0; }

int32_t svthip_av1_wiener_stats_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t plane_start, uint32_t plane_end, int64_t* d_M,
                                    int64_t* d_H, int32_t* d_avg, int64_t* d_sse_none, void* d_work, void* stream)
{
    TRY(enter(ctx));
    return lr_stats_entry(ctx, picture, plane_start, plane_end, 8, d_M, d_H, d_avg, d_sse_none, d_work, stream);
}

int32_t svthip_av1_highbd_wiener_stats_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t plane_start, uint32_t plane_end,
                                           uint32_t bit_depth, int64_t* d_M, int64_t* d_H, int32_t* d_avg, int64_t* d_sse_none, void* d_work,
                                           void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return lr_stats_entry(ctx, picture, plane_start, plane_end, 10, d_M, d_H, d_avg, d_sse_none, d_work, stream);
}

int32_t svthip_wiener_solve_dev(svthip_ctx* ctx, const int64_t* d_M, const int64_t* d_H, uint32_t unit_begin, uint32_t unit_end, uint32_t wiener_win,
                                int16_t* d_taps, int32_t* d_rejected, void* stream)
{
    TRY(enter(ctx));
    TRY(check_lr_units(unit_begin, unit_end, wiener_win));
    TRY(check_non_null({d_M, d_H, d_taps, d_rejected}));
    if (!aligned({d_M, d_H}, 8) || !aligned(d_rejected, 4) || !aligned(d_taps, 2))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "d_M and d_H must be 8-byte, d_rejected 4-byte, d_taps 2-byte aligned");
    HIP_TRY(svthip::launch_lr_solve(d_M, d_H, unit_begin, unit_end, (int)wiener_win, d_taps, d_rejected, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t svthip_av1_wiener_trial_sse_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t plane_start, uint32_t plane_end,
                                        const int16_t* d_taps, const uint8_t* d_skip, int64_t* d_sse, void* stream)
{
    TRY(enter(ctx));
    return lr_trial_entry(ctx, picture, plane_start, plane_end, 8, d_taps, d_skip, d_sse, stream);
}

int32_t svthip_av1_highbd_wiener_trial_sse_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t plane_start, uint32_t plane_end,
                                               uint32_t bit_depth, const int16_t* d_taps, const uint8_t* d_skip, int64_t* d_sse, void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return lr_trial_entry(ctx, picture, plane_start, plane_end, 10, d_taps, d_skip, d_sse, stream);
}

int32_t svthip_wiener_walk_init_dev(svthip_ctx* ctx, svthip_wiener_walk_state* d_state, const int16_t* d_taps, const int32_t* d_rejected,
                                    uint32_t unit_begin, uint32_t unit_end, uint32_t wiener_win, void* stream)
{
    TRY(enter(ctx));
    TRY(check_lr_units(unit_begin, unit_end, wiener_win));
    TRY(check_non_null({d_state, d_taps}));
    if (!aligned(d_state, 8) || !aligned(d_rejected, 4) || !aligned(d_taps, 2))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "d_state must be 8-byte, d_rejected 4-byte, d_taps 2-byte aligned");
    HIP_TRY(svthip::launch_lr_walk_init(d_state, d_taps, d_rejected, unit_begin, unit_end, (int)wiener_win, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t svthip_wiener_walk_step_dev(svthip_ctx* ctx, svthip_wiener_walk_state* d_state, const int64_t* d_trial_sse, uint32_t unit_begin,
                                    uint32_t unit_end, int32_t* d_pending, void* stream)
{
    TRY(enter(ctx));
    TRY(check_lr_units(unit_begin, unit_end, 7));
    TRY(check_non_null({d_state, d_trial_sse}));
    if (!aligned({d_state, d_trial_sse}, 8) || !aligned(d_pending, 4))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "d_state and d_trial_sse must be 8-byte, d_pending 4-byte aligned");
    HIP_TRY(svthip::launch_lr_walk_step(d_state, d_trial_sse, unit_begin, unit_end, d_pending, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t svthip_av1_search_wiener_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t plane_start, uint32_t plane_end, uint32_t n_steps,
                                     uint32_t resume, void* d_work, int64_t* d_sse, int16_t* d_taps, int32_t* d_n_trials, int32_t* d_pending,
                                     void* stream)
{
    TRY(enter(ctx));
    return lr_search_entry(ctx, picture, plane_start, plane_end, 8, n_steps, resume, d_work, d_sse, d_taps, d_n_trials, d_pending, stream);
}

int32_t svthip_av1_highbd_search_wiener_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t plane_start, uint32_t plane_end,
                                            uint32_t bit_depth, uint32_t n_steps, uint32_t resume, void* d_work, int64_t* d_sse, int16_t* d_taps,
                                            int32_t* d_n_trials, int32_t* d_pending, void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return lr_search_entry(ctx, picture, plane_start, plane_end, 10, n_steps, resume, d_work, d_sse, d_taps, d_n_trials, d_pending, stream);
}

int32_t svthip_av1_loop_restoration_filter_frame_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, void* const d_out[3],
                                                     const uint32_t out_stride[3], uint32_t plane_start, uint32_t plane_end,
                                                     const uint8_t* d_unit_type, const int16_t* d_taps, void* stream)
{
    TRY(enter(ctx));
    return lr_filter_frame_entry(ctx, picture, d_out, out_stride, plane_start, plane_end, 8, d_unit_type, d_taps, nullptr, false, stream);
}

int32_t svthip_av1_highbd_loop_restoration_filter_frame_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, void* const d_out[3],
                                                            const uint32_t out_stride[3], uint32_t plane_start, uint32_t plane_end,
                                                            uint32_t bit_depth, const uint8_t* d_unit_type, const int16_t* d_taps, void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return lr_filter_frame_entry(ctx, picture, d_out, out_stride, plane_start, plane_end, 10, d_unit_type, d_taps, nullptr, false, stream);
}

// Self-guided loop restoration (Codec/EbRestorationPick.c:248-670, :1670-1706; EbRestoration.c:731-1246): the box filter over a plane, the
// projection solve, the walk on a table, the whole search, the SSE trial, and the frame filter for all three unit types
size_t svthip_sgrproj_workspace_bytes(uint32_t width, uint32_t height) { return svthip::sgr_workspace(width, height).total; }

uint32_t svthip_sgrproj_walk_max_trials(void) { return svthip::sgr_walk_max_trials(); }

int32_t svthip_av1_selfguided_restoration_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t plane, uint32_t ep, int32_t* d_flt0,
                                              int32_t* d_flt1, uint32_t flt_stride, void* stream)
{
    TRY(enter(ctx));
    return sgr_plane_entry(ctx, picture, plane, 8, ep, d_flt0, d_flt1, flt_stride, stream);
}

int32_t svthip_av1_highbd_selfguided_restoration_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t plane, uint32_t bit_depth, uint32_t ep,
                                                     int32_t* d_flt0, int32_t* d_flt1, uint32_t flt_stride, void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return sgr_plane_entry(ctx, picture, plane, 10, ep, d_flt0, d_flt1, flt_stride, stream);
}

int32_t svthip_sgrproj_solve_dev(svthip_ctx* ctx, const int64_t* d_sums, const int32_t* d_size, const int32_t* d_ep, uint32_t n, int32_t* d_xq,
                                 int32_t* d_xqd, void* stream)
{
    TRY(enter(ctx));
    TRY(check_non_null({d_sums, d_size, d_ep, d_xq, d_xqd}));
    if (!aligned(d_sums, 8) || !aligned({d_size, d_ep, d_xq, d_xqd}, 4))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "d_sums must be 8-byte, d_size, d_ep, d_xq and d_xqd 4-byte aligned");
    HIP_TRY(svthip::launch_sgr_solve(d_sums, d_size, d_ep, n, d_xq, d_xqd, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t svthip_sgrproj_walk_table_dev(svthip_ctx* ctx, const int64_t* d_err, const int32_t* d_ep, const int32_t* d_start_xqd, uint32_t n, int32_t* d_xqd,
                                      int64_t* d_best_err, int32_t* d_n_trials, void* stream)
{
    TRY(enter(ctx));
    TRY(check_non_null({d_err, d_ep, d_start_xqd, d_xqd, d_best_err, d_n_trials}));
    if (!aligned({d_err, d_best_err}, 8) || !aligned({d_ep, d_start_xqd, d_xqd, d_n_trials}, 4))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "d_err and d_best_err must be 8-byte, d_ep, d_start_xqd, d_xqd and d_n_trials 4-byte aligned");
    HIP_TRY(svthip::launch_sgr_walk_table(d_err, d_ep, d_start_xqd, n, d_xqd, d_best_err, d_n_trials, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t svthip_av1_search_sgrproj_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t plane_start, uint32_t plane_end, void* d_work,
                                      int32_t* d_sgrproj, int64_t* d_sse, svthip_sgrproj_detail* d_detail, void* stream)
{
    TRY(enter(ctx));
    return sgr_search_entry(ctx, picture, plane_start, plane_end, 8, d_work, d_sgrproj, d_sse, d_detail, stream);
}

int32_t svthip_av1_highbd_search_sgrproj_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t plane_start, uint32_t plane_end,
                                             uint32_t bit_depth, void* d_work, int32_t* d_sgrproj, int64_t* d_sse, svthip_sgrproj_detail* d_detail,
                                             void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return sgr_search_entry(ctx, picture, plane_start, plane_end, 10, d_work, d_sgrproj, d_sse, d_detail, stream);
}

int32_t svthip_av1_sgrproj_trial_sse_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t plane_start, uint32_t plane_end,
                                         const int32_t* d_sgrproj, const uint8_t* d_skip, int64_t* d_sse, void* stream)
{
    TRY(enter(ctx));
    return sgr_trial_entry(ctx, picture, plane_start, plane_end, 8, d_sgrproj, d_skip, d_sse, stream);
}

int32_t svthip_av1_highbd_sgrproj_trial_sse_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t plane_start, uint32_t plane_end,
                                                uint32_t bit_depth, const int32_t* d_sgrproj, const uint8_t* d_skip, int64_t* d_sse, void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return sgr_trial_entry(ctx, picture, plane_start, plane_end, 10, d_sgrproj, d_skip, d_sse, stream);
}

int32_t svthip_av1_lr_filter_frame_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, void* const d_out[3], const uint32_t out_stride[3],
                                       uint32_t plane_start, uint32_t plane_end, const uint8_t* d_unit_type, const int16_t* d_taps,
                                       const int32_t* d_sgrproj, void* stream)
{
    TRY(enter(ctx));
    return lr_filter_frame_entry(ctx, picture, d_out, out_stride, plane_start, plane_end, 8, d_unit_type, d_taps, d_sgrproj, true, stream);
}

int32_t svthip_av1_highbd_lr_filter_frame_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, void* const d_out[3], const uint32_t out_stride[3],
                                              uint32_t plane_start, uint32_t plane_end, uint32_t bit_depth, const uint8_t* d_unit_type,
                                              const int16_t* d_taps, const int32_t* d_sgrproj, void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return lr_filter_frame_entry(ctx, picture, d_out, out_stride, plane_start, plane_end, 10, d_unit_type, d_taps, d_sgrproj, true, stream);
}

size_t svthip_lr_pick_workspace_bytes(uint32_t width, uint32_t height, const uint32_t unit_size[3])
{
    if (!unit_size || width == 0 || height == 0 || (width | height) % 8 != 0 || width > 16384 || height > 16384) return 0;
    for (int p = 0; p < 3; p++)
        if (unit_size[p] != 64 && unit_size[p] != 128 && unit_size[p] != 256) return 0;
    return svthip::lr_pick_workspace(width, height, unit_size).total;
}

int32_t svthip_rest_finish_search_dev(svthip_ctx* ctx, const svthip_rest_finish_rates* rates, const uint32_t unit_base[4], uint32_t plane_start,
                                      uint32_t plane_end, const int64_t* d_wiener_sse, const int16_t* d_taps, const int64_t* d_sgr_sse,
                                      const int32_t* d_sgrproj, uint8_t* d_unit_type, uint8_t* d_best_rtype, svthip_rest_finish_result* d_result,
                                      void* stream)
{
    TRY(enter(ctx));
    TRY(check_rest_finish_rates(rates));
    TRY(check_non_null({unit_base, d_wiener_sse, d_taps, d_sgr_sse, d_sgrproj, d_unit_type, d_result}));
    if (plane_start >= plane_end || plane_end > 3)
        return fail(SVTHIP_ERR_BAD_PARAMETER, "planes [%u, %u) are empty or not within 0..3", (unsigned)plane_start, (unsigned)plane_end);
    for (uint32_t p = 0; p < 3; p++) {
        if (unit_base[p] > unit_base[p + 1]) return fail(SVTHIP_ERR_BAD_PARAMETER, "unit_base does not ascend at plane %d", (int)p);
        if (p >= plane_start && p < plane_end && unit_base[p] == unit_base[p + 1])
            return fail(SVTHIP_ERR_BAD_PARAMETER, "plane %d has no unit", (int)p);
    }
    if (!aligned({d_wiener_sse, d_sgr_sse, d_result}, 8) || !aligned(d_sgrproj, 4) || !aligned(d_taps, 2))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "d_wiener_sse, d_sgr_sse and d_result must be 8-byte, d_sgrproj 4-byte, d_taps 2-byte aligned");
    hipStream_t s;
    uint32_t* d_refused;
    TRY(refused_counter(ctx, stream, &s, &d_refused));
    HIP_TRY(svthip::launch_rest_finish(*rates, unit_base, (int)plane_start, (int)plane_end, d_wiener_sse, d_taps, d_sgr_sse, d_sgrproj, d_unit_type,
                                       d_best_rtype, d_result, d_refused, s));
    return SVTHIP_OK;
}

int32_t svthip_av1_pick_filter_restoration_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, const svthip_rest_finish_rates* rates, void* d_work,
                                               void* const d_out[3], const uint32_t out_stride[3], uint8_t* d_unit_type, int16_t* d_taps,
                                               int32_t* d_sgrproj, svthip_rest_finish_result* d_result, void* stream)
{
    TRY(enter(ctx));
    return lr_pick_filter_entry(ctx, picture, 8, rates, d_work, d_out, out_stride, d_unit_type, d_taps, d_sgrproj, d_result, stream);
}

int32_t svthip_av1_highbd_pick_filter_restoration_dev(svthip_ctx* ctx, const svthip_lr_picture* picture, uint32_t bit_depth,
                                                      const svthip_rest_finish_rates* rates, void* d_work, void* const d_out[3],
                                                      const uint32_t out_stride[3], uint8_t* d_unit_type, int16_t* d_taps, int32_t* d_sgrproj,
                                                      svthip_rest_finish_result* d_result, void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return lr_pick_filter_entry(ctx, picture, 10, rates, d_work, d_out, out_stride, d_unit_type, d_taps, d_sgrproj, d_result, stream);
}

}  // extern "C"
