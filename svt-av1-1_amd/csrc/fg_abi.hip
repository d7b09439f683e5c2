// svt-av1-1_amd/csrc/fg_abi.hip -- C-ABI glue of film-grain synthesis: the exported entries that launch through
// fg_launch.h, with their validators and shared bodies.  Host code only.
#include "svthip_glue.h"
#include "fg_launch.h"

namespace {

// every range the kernels rely on (the parameter block is narrowed to bytes after this) and every value the reference would divide by
int32_t check_film_grain_params(const svthip_film_grain_params* p)
{
    const struct { const char* name; const int32_t (*points)[2]; int32_t n, max; } planes[3] = {
        {"y", p->scaling_points_y, p->num_y_points, 14}, {"cb", p->scaling_points_cb, p->num_cb_points, 10}, {"cr", p->scaling_points_cr, p->num_cr_points, 10}};
    for (const auto& pl : planes) {
        if (pl.n < 0 || pl.n > pl.max) return fail(SVTHIP_ERR_BAD_PARAMETER, "num_%s_points must be 0..%d (got %d)", pl.name, (int)pl.max, (int)pl.n);
        for (int i = 0; i < pl.n; i++) {
            const int32_t x = pl.points[i][0], y = pl.points[i][1];
            if (x < 0 || x > 255 || y < 0 || y > 255 || (i && x <= pl.points[i - 1][0]))
                return fail(SVTHIP_ERR_BAD_PARAMETER, "scaling_points_%s[%d] = (%d, %d): x must increase strictly, x and y lie in 0..255", pl.name, i, (int)x, (int)y);
        }
    }
    if (p->scaling_shift < 8 || p->scaling_shift > 11) return fail(SVTHIP_ERR_BAD_PARAMETER, "scaling_shift must be 8..11 (got %d)", (int)p->scaling_shift);
    if (p->ar_coeff_lag < 0 || p->ar_coeff_lag > 3) return fail(SVTHIP_ERR_BAD_PARAMETER, "ar_coeff_lag must be 0..3 (got %d)", (int)p->ar_coeff_lag);
    if (p->ar_coeff_shift < 6 || p->ar_coeff_shift > 9) return fail(SVTHIP_ERR_BAD_PARAMETER, "ar_coeff_shift must be 6..9 (got %d)", (int)p->ar_coeff_shift);
    if (p->grain_scale_shift < 0 || p->grain_scale_shift > 3)
        return fail(SVTHIP_ERR_BAD_PARAMETER, "grain_scale_shift must be 0..3 (got %d)", (int)p->grain_scale_shift);
    const int32_t* coeffs[3] = {p->ar_coeffs_y, p->ar_coeffs_cb, p->ar_coeffs_cr};
    for (int k = 0; k < 3; k++)
        for (int i = 0; i < (k ? 25 : 24); i++)
            if (coeffs[k][i] < -128 || coeffs[k][i] > 127)
                return fail(SVTHIP_ERR_BAD_PARAMETER, "AR coefficient %d of plane %d must be -128..127 (got %d)", i, k, (int)coeffs[k][i]);
    for (int32_t m : {p->cb_mult, p->cb_luma_mult, p->cr_mult, p->cr_luma_mult})
        if (m < 0 || m > 255) return fail(SVTHIP_ERR_BAD_PARAMETER, "cb_mult, cb_luma_mult, cr_mult and cr_luma_mult must be 0..255 (got %d)", (int)m);
    for (int32_t o : {p->cb_offset, p->cr_offset})
        if (o < 0 || o > 511) return fail(SVTHIP_ERR_BAD_PARAMETER, "cb_offset and cr_offset must be 0..511 (got %d)", (int)o);
    return SVTHIP_OK;
}

int32_t add_film_grain_entry(svthip_ctx* ctx, const svthip_film_grain_params* params, const void* const d_src[3], const uint32_t src_stride[3],
                             void* const d_dst[3], const uint32_t dst_stride[3], uint32_t width, uint32_t height, int bd, const int16_t* d_tables,
                             void* stream)
{
    TRY(check_non_null({params, d_src, src_stride, d_dst, dst_stride}));
    if ((width & 1) || (height & 1) || !width || !height || width > 65536 || height > 65536)
        return fail(SVTHIP_ERR_BAD_PARAMETER, "picture dimensions must be even, 2..65536 (%ux%u)", (unsigned)width, (unsigned)height);
    for (int p = 0; p < 3; p++) {
        TRY(check_non_null({d_src[p], d_dst[p]}));
        if (d_src[p] == d_dst[p]) return fail(SVTHIP_ERR_BAD_PARAMETER, "film grain is added out of place: d_dst[%d] == d_src[%d]", p, p);
        const uint32_t w = p ? width / 2 : width;
        if (src_stride[p] < w || dst_stride[p] < w) return fail(SVTHIP_ERR_BAD_PARAMETER, "the strides of plane %d must be >= its width %u", p, (unsigned)w);
        if (bd > 8 && !aligned({d_src[p], d_dst[p]}, 2)) return fail(SVTHIP_ERR_BAD_PARAMETER, "16-bit planes must be 2-byte aligned (plane %d)", p);
    }
    if (d_tables && !aligned(d_tables, 2)) return fail(SVTHIP_ERR_BAD_PARAMETER, "d_tables must be 2-byte aligned");
    TRY(check_film_grain_params(params));
    hipStream_t s = call_stream(ctx, stream);
    if (!d_tables) {
        TRY(ensure_scratch(ctx, SLOT_FILM_GRAIN_TABLES, SVTHIP_FILM_GRAIN_TABLES_BYTES));
        TRY(scratch_on_stream(ctx, s));
        HIP_TRY(svthip::launch_film_grain_tables(*params, bd, slot_ptr<int16_t>(ctx, SLOT_FILM_GRAIN_TABLES), s));
        d_tables = slot_ptr<int16_t>(ctx, SLOT_FILM_GRAIN_TABLES);
    }
    HIP_TRY(svthip::launch_film_grain_frame(*params, bd, d_src, src_stride, d_dst, dst_stride, width, height, d_tables, s));
    return SVTHIP_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- film grain

int32_t svthip_film_grain_tables_dev(svthip_ctx* ctx, const svthip_film_grain_params* params, uint32_t bit_depth, int16_t* d_tables, void* stream)
{
    TRY(enter(ctx));
    TRY(check_non_null({params, d_tables}));
    if (bit_depth != 8 && bit_depth != 10) return fail(SVTHIP_ERR_BAD_PARAMETER, "bit_depth must be 8 or 10 (got %d)", (int)bit_depth);
    if (!aligned(d_tables, 2)) return fail(SVTHIP_ERR_BAD_PARAMETER, "d_tables must be 2-byte aligned");
    TRY(check_film_grain_params(params));
    HIP_TRY(svthip::launch_film_grain_tables(*params, (int)bit_depth, d_tables, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t svthip_av1_add_film_grain_dev(svthip_ctx* ctx, const svthip_film_grain_params* params, const void* const d_src[3], const uint32_t src_stride[3],
                                      void* const d_dst[3], const uint32_t dst_stride[3], uint32_t width, uint32_t height, const int16_t* d_tables,
                                      void* stream)
{
    TRY(enter(ctx));
    return add_film_grain_entry(ctx, params, d_src, src_stride, d_dst, dst_stride, width, height, 8, d_tables, stream);
}

int32_t svthip_av1_highbd_add_film_grain_dev(svthip_ctx* ctx, const svthip_film_grain_params* params, const void* const d_src[3],
                                             const uint32_t src_stride[3], void* const d_dst[3], const uint32_t dst_stride[3], uint32_t width,
                                             uint32_t height, uint32_t bit_depth, const int16_t* d_tables, void* stream)
{
    TRY(enter(ctx));
    TRY(check_bit_depth_10(bit_depth));
    return add_film_grain_entry(ctx, params, d_src, src_stride, d_dst, dst_stride, width, height, 10, d_tables, stream);
}

}  // extern "C"
