// svt-av1-1_amd/csrc/md_abi.hip -- C-ABI glue of mode decision: the exported entries that launch through
// md_launch.h, with their validators.  Host code only.
#include "svthip_glue.h"
#include "ip_launch.h"  // inter_pred_scratch_bytes: the interpolation-filter search predicts its trial tiles with the inter-prediction kernels
#include "md_launch.h"

namespace {

int32_t check_md_ifs_size(uint32_t bwidth, uint32_t bheight)
{
    if (!svthip::md_ifs_size_ok(bwidth, bheight))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "not one of the 17 AV1 block sizes with both sides above 4 (%d x %d)", (int)bwidth, (int)bheight);
    return SVTHIP_OK;
}
int32_t check_md_ifs_quantizer(int32_t quantizer)   // the reference's int16_t, an int32_t in the ABI
{
    if (quantizer < -32768 || quantizer > 32767) return fail(SVTHIP_ERR_BAD_PARAMETER, "quantizer %d is not an int16_t value", (int)quantizer);
    return SVTHIP_OK;
}

// the two full-loop entries: `wide` takes 128x128, 128x64 and 64x128 and has d_tu, the other takes the 19 sizes with both sides <= 64
int32_t md_full_loop(bool wide, svthip_ctx* ctx, const svthip_inter_planes* src, const svthip_inter_planes* pred, const svthip_md_fast_desc* d_fast,
                     const svthip_md_full_desc* d_full, uint32_t n_cand, const svthip_md_fast_group* d_group, const svthip_md_fast_pick* d_pick,
                     uint32_t n_groups, uint32_t bwidth, uint32_t bheight, const int16_t* d_qparams, const int16_t* d_iscan, const uint32_t* iscan_offsets,
                     const svthip_coeff_rate_tables* d_tables, int32_t reduced_tx_set, uint32_t type_mask_inter, uint32_t type_mask_intra, uint32_t max_full,
                     const svthip_inter_planes* slot_recon, uint32_t tiles_per_row, const svthip_inter_planes* recon, void* d_work, uint32_t stages,
                     svthip_md_full_result* d_result, svthip_md_full128_tu* d_tu, svthip_md_full_decision* d_decision, void* stream)
{
    TRY(enter(ctx));
    if (!svthip::md_full_size_ok(bwidth, bheight, wide))
        return fail(SVTHIP_ERR_BAD_PARAMETER, wide ? "not one of the block sizes 128x128, 128x64 and 64x128 (%d x %d)"
                                                   : "not one of the 19 AV1 block sizes with both sides up to 64 (%d x %d)", (int)bwidth, (int)bheight);
    const uint32_t all_stages = SVTHIP_MD_FULL_LUMA | SVTHIP_MD_FULL_CHROMA | SVTHIP_MD_FULL_DECIDE;
    if (!stages || (stages & ~all_stages)) return fail(SVTHIP_ERR_BAD_PARAMETER, "stages must be a mask of SVTHIP_MD_FULL_LUMA, _CHROMA, _DECIDE (got %d)", (int)stages);
    if (max_full < 1 || max_full > SVTHIP_MD_FULL_MAX_SLOTS) return fail(SVTHIP_ERR_BAD_PARAMETER, "max_full must be 1..12 (got %d)", (int)max_full);
    if (!tiles_per_row) return fail(SVTHIP_ERR_BAD_PARAMETER, "tiles_per_row must not be 0");
    svthip::MdFullLayout L;
    if (!type_mask_inter || !type_mask_intra || ((type_mask_inter | type_mask_intra) >> 16) ||
        !svthip::md_full_layout(0, max_full, bwidth, bheight, wide, type_mask_inter, type_mask_intra, &L))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "a type mask is 0, has bits above 15 or names a TxType %d x %d has no network for (0x%x, 0x%x)", (int)bwidth,
                    (int)bheight, (unsigned)type_mask_inter, (unsigned)type_mask_intra);
    if (n_groups == 0) return SVTHIP_OK;
    TRY(pred_check_args({src, pred, slot_recon, recon}, d_fast));
    TRY(check_non_null({d_full, d_group, d_pick, d_qparams, d_iscan, iscan_offsets, d_tables, d_work, d_result, d_decision}));
    if (wide) {
        TRY(check_non_null({d_tu}));
    }
    if (n_cand == 0) return fail(SVTHIP_ERR_BAD_PARAMETER, "n_cand must not be 0: an inactive slot repeats row 0");
    if (!aligned({d_full, d_pick, d_work, d_result, d_decision, d_tu}, 16))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "descriptor, pick, workspace, result and decision arrays must be 16-byte aligned");
    if (!aligned(d_group, 8)) return fail(SVTHIP_ERR_BAD_PARAMETER, "group array must be 8-byte aligned");
    if (!aligned(d_qparams, 2) || !aligned(d_tables, 4)) return fail(SVTHIP_ERR_BAD_PARAMETER, "qparams must be 2-byte, tables 4-byte aligned");
    TRY(check_tq_pools(nullptr, nullptr, nullptr, d_iscan));
    for (const svthip_inter_planes* p : {src, pred, slot_recon, recon})
        if (p->y_stride > 65535u || p->c_stride > 65535u)
            return fail(SVTHIP_ERR_BAD_PARAMETER, "plane strides must be at most 65535: a TU descriptor holds 16-bit strides (got %u)",
                        (unsigned)(p->y_stride > p->c_stride ? p->y_stride : p->c_stride));
    const uint64_t n_slots = (uint64_t)n_groups * max_full;
    const uint64_t tile_w = bwidth < 8 ? 8 : bwidth, tile_h = bheight < 8 ? 8 : bheight, tile_rows = (n_slots + tiles_per_row - 1) / tiles_per_row;
    if (!svthip::md_full_layout(n_groups, max_full, bwidth, bheight, wide, type_mask_inter, type_mask_intra, &L) || tiles_per_row * tile_w > 65535u ||
        tile_rows * tile_h * slot_recon->y_stride > 0xffffffffull)
        return fail(SVTHIP_ERR_BAD_PARAMETER, "too many slots in one call (%d groups of %d): their tiles or coefficients pass 32-bit offsets", (int)n_groups,
                    (int)max_full);
    hipStream_t s;
    uint32_t* d_refused;
    TRY(refused_counter(ctx, stream, &s, &d_refused));
    svthip::MdFullCall call = {*src, *pred, *slot_recon, *recon, d_fast, d_full, d_group, d_pick, n_cand, n_groups, bwidth, bheight, max_full, tiles_per_row,
                               type_mask_inter, type_mask_intra, stages, reduced_tx_set, d_qparams, d_iscan, iscan_offsets, d_tables, d_work, d_result,
                               d_decision, d_refused, (uint32_t)ctx->opt[SVTHIP_OPT_TQ_MAX_WORKGROUPS], d_tu};
    HIP_TRY(svthip::launch_md_full_loop(call, L, s));
    return SVTHIP_OK;
}

// The three partition entries: `decide` and `compose` say which launches run.  What needs no device is checked before the context is
// entered, so a refusal does not depend on one.
int32_t md_partition(bool decide, bool compose, svthip_ctx* ctx, const svthip::MdPartCall& C, const svthip_inter_planes* pool, const svthip_inter_planes* dst,
                     void* stream)
{
    if (C.sb_size != 64u && C.sb_size != 128u) return fail(SVTHIP_ERR_BAD_PARAMETER, "sb_size must be 64 or 128 (got %d)", (int)C.sb_size);
    if (C.n_sb) {
        TRY(check_non_null({C.leaf, C.final_, C.final_count}));
        if (!aligned({C.leaf, C.final_}, 16) || !aligned(C.final_count, 4))
            return fail(SVTHIP_ERR_BAD_PARAMETER, "leaf and final-block arrays must be 16-byte aligned, the final counts 4-byte");
        if (decide) {
            TRY(check_non_null({C.sb, C.decision, C.partition_fac_bits, C.result}));
            if (!aligned({C.sb, C.decision, C.result}, 16))
                return fail(SVTHIP_ERR_BAD_PARAMETER, "superblock, decision and result arrays must be 16-byte aligned");
        }
        if (compose) {
            TRY(check_non_null({pool, dst}));
            TRY(check_non_null({pool->y, pool->cb, pool->cr, dst->y, dst->cb, dst->cr}));
            if (!C.width || !C.height || !C.pool_width || !C.pool_height)
                return fail(SVTHIP_ERR_BAD_PARAMETER, "picture and pool sizes must not be 0 (%d x %d, %d x %d)", (int)C.width, (int)C.height, (int)C.pool_width,
                            (int)C.pool_height);
            if (pool->y_stride < C.pool_width || pool->c_stride < (C.pool_width + 1u) / 2u || dst->y_stride < C.width || dst->c_stride < (C.width + 1u) / 2u)
                return fail(SVTHIP_ERR_BAD_PARAMETER, "a plane stride is below the width of its plane");
        }
    }
    TRY(enter(ctx));
    if (C.n_sb == 0) return SVTHIP_OK;
    svthip::MdPartCall call = C;
    if (compose) call.pool = *pool, call.dst = *dst;
    hipStream_t s;
    TRY(refused_counter(ctx, stream, &s, &call.refused));
    if (decide) HIP_TRY(svthip::launch_md_part_decide(call, s));
    if (compose) HIP_TRY(svthip::launch_md_part_compose(call, s));
    return SVTHIP_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- mode decision's fast loop

int32_t svthip_md_fast_cost_batch_dev(svthip_ctx* ctx, const svthip_inter_planes* src, const svthip_inter_planes* pred, const svthip_md_fast_desc* d_desc,
                                      uint32_t n_cand, uint32_t bwidth, uint32_t bheight, svthip_md_fast_result* d_result, void* stream)
{
    TRY(enter(ctx));
    TRY(check_av1_block(bwidth, bheight));
    if (n_cand == 0) return SVTHIP_OK;
    TRY(pred_check_args({src, pred}, d_desc));   // has_uv is device data: every call may touch chroma, so no plane may be null
    TRY(check_non_null({d_result}));
    if (!aligned(d_result, 16)) return fail(SVTHIP_ERR_BAD_PARAMETER, "result array must be 16-byte aligned");
    HIP_TRY(svthip::launch_md_fast_cost(*src, *pred, d_desc, n_cand, bwidth, bheight, d_result, call_stream(ctx, stream)));
    return SVTHIP_OK;
}

int32_t svthip_md_fast_pick_batch_dev(svthip_ctx* ctx, const svthip_md_fast_result* d_result, const svthip_md_fast_desc* d_desc, uint32_t n_cand,
                                      const svthip_md_fast_group* d_group, uint32_t n_groups, svthip_md_fast_pick* d_pick, void* stream)
{
    TRY(enter(ctx));
    if (n_groups == 0) return SVTHIP_OK;
    TRY(check_non_null({d_result, d_desc, d_group, d_pick}));
    if (!aligned({d_result, d_desc, d_pick}, 16)) return fail(SVTHIP_ERR_BAD_PARAMETER, "result, descriptor and pick arrays must be 16-byte aligned");
    if (!aligned(d_group, 8)) return fail(SVTHIP_ERR_BAD_PARAMETER, "group array must be 8-byte aligned");
    hipStream_t s;
    uint32_t* d_refused;
    TRY(refused_counter(ctx, stream, &s, &d_refused));
    HIP_TRY(svthip::launch_md_fast_pick(d_result, d_desc, n_cand, d_group, n_groups, d_pick, d_refused, s));
    return SVTHIP_OK;
}

// ---------------------------------------------------------------- mode decision's interpolation-filter search

int32_t svthip_md_model_rd_batch_dev(svthip_ctx* ctx, const svthip_inter_planes* src, const svthip_inter_planes* pred, const svthip_md_model_rd_desc* d_desc,
                                     uint32_t n_tiles, uint32_t bwidth, uint32_t bheight, int32_t quantizer, svthip_md_model_rd_result* d_result, void* stream)
{
    TRY(enter(ctx));
    TRY(check_md_ifs_size(bwidth, bheight));
    TRY(check_md_ifs_quantizer(quantizer));
    if (n_tiles == 0) return SVTHIP_OK;
    TRY(pred_check_args({src, pred}, d_desc));
    TRY(check_non_null({d_result}));
    if (!aligned(d_result, 16)) return fail(SVTHIP_ERR_BAD_PARAMETER, "result array must be 16-byte aligned");
    hipStream_t s;
    uint32_t* d_refused;
    TRY(refused_counter(ctx, stream, &s, &d_refused));
    HIP_TRY(svthip::launch_md_model_rd(*src, *pred, d_desc, n_tiles, bwidth, bheight, (int16_t)quantizer, d_result, d_refused, s));
    return SVTHIP_OK;
}

int32_t svthip_md_interp_filter_search_batch_dev(svthip_ctx* ctx, const svthip_inter_planes* ref0, const svthip_inter_planes* ref1,
                                                 const svthip_inter_planes* src, svthip_inter_pu_desc* d_pu_desc, const svthip_md_ifs_desc* d_ifs_desc,
                                                 uint32_t n_cand, uint32_t bwidth, uint32_t bheight, int32_t search_mode, int32_t enable_dual_filter,
                                                 int32_t quantizer, int32_t write_back, svthip_md_ifs_result* d_result, void* stream)
{
    TRY(enter(ctx));
    TRY(check_md_ifs_size(bwidth, bheight));
    if (search_mode != 1 && search_mode != 2) return fail(SVTHIP_ERR_BAD_PARAMETER, "search_mode must be 1 (fast) or 2 (full), not %d", (int)search_mode);
    TRY(check_md_ifs_quantizer(quantizer));
    if (n_cand == 0) return SVTHIP_OK;
    TRY(pred_check_args({ref0, ref1, src}, d_pu_desc));
    TRY(check_non_null({d_ifs_desc, d_result}));
    if (!aligned({d_ifs_desc, d_result}, 16)) return fail(SVTHIP_ERR_BAD_PARAMETER, "search descriptor and result arrays must be 16-byte aligned");
    const uint64_t n_tiles = (uint64_t)n_cand * svthip::md_ifs_trials(search_mode, enable_dual_filter);
    svthip::MdIfsLayout L;
    if (n_tiles > 0x0fffffffu || !svthip::md_ifs_layout(n_tiles, bwidth, bheight, &L))
        return fail(SVTHIP_ERR_BAD_PARAMETER, "too many candidates in one call (%d): their trial tiles pass what 16-bit tile positions address", (int)n_cand);
    hipStream_t s;
    uint32_t* d_refused;
    TRY(pred_begin(ctx, {ref0, ref1, src}, 8, (uint32_t)n_tiles, 0x0fffffffu, svthip::inter_pred_scratch_bytes, stream, &s, &d_refused));
    TRY(ensure_scratch(ctx, SLOT_MD_IFS, L.total));
    HIP_TRY(svthip::launch_md_ifs_search(*ref0, *ref1, *src, d_pu_desc, d_ifs_desc, n_cand, bwidth, bheight, search_mode, enable_dual_filter, (int16_t)quantizer,
                                         write_back, d_result, !ctx->opt[SVTHIP_OPT_CONVOLVE_VALU], ctx->scratch[SLOT_MD_IFS], L,
                                         ctx->scratch[SLOT_INTER_JOBS], d_refused, s));
    return SVTHIP_OK;
}

// ---------------------------------------------------------------- mode decision's full loop

size_t svthip_md_full_workspace_bytes(uint32_t n_groups, uint32_t max_full, uint32_t bwidth, uint32_t bheight, uint32_t type_mask_inter,
                                      uint32_t type_mask_intra)
{
    svthip::MdFullLayout L;
    return svthip::md_full_layout(n_groups, max_full, bwidth, bheight, false, type_mask_inter, type_mask_intra, &L) ? L.total : 0;
}

int32_t svthip_md_full_loop_batch_dev(svthip_ctx* ctx, const svthip_inter_planes* src, const svthip_inter_planes* pred, const svthip_md_fast_desc* d_fast,
                                      const svthip_md_full_desc* d_full, uint32_t n_cand, const svthip_md_fast_group* d_group,
                                      const svthip_md_fast_pick* d_pick, uint32_t n_groups, uint32_t bwidth, uint32_t bheight, const int16_t* d_qparams,
                                      const int16_t* d_iscan, const uint32_t iscan_offsets[19 * 16], const svthip_coeff_rate_tables* d_tables,
                                      int32_t reduced_tx_set, uint32_t type_mask_inter, uint32_t type_mask_intra, uint32_t max_full,
                                      const svthip_inter_planes* slot_recon, uint32_t tiles_per_row, const svthip_inter_planes* recon, void* d_work,
                                      uint32_t stages, svthip_md_full_result* d_result, svthip_md_full_decision* d_decision, void* stream)
{
    return md_full_loop(false, ctx, src, pred, d_fast, d_full, n_cand, d_group, d_pick, n_groups, bwidth, bheight, d_qparams, d_iscan, iscan_offsets, d_tables,
                        reduced_tx_set, type_mask_inter, type_mask_intra, max_full, slot_recon, tiles_per_row, recon, d_work, stages, d_result, nullptr,
                        d_decision, stream);
}

size_t svthip_md_full128_workspace_bytes(uint32_t n_groups, uint32_t max_full, uint32_t bwidth, uint32_t bheight)
{
    svthip::MdFullLayout L;
    return svthip::md_full_layout(n_groups, max_full, bwidth, bheight, true, 1, 1, &L) ? L.total : 0;
}

int32_t svthip_md_full_loop128_batch_dev(svthip_ctx* ctx, const svthip_inter_planes* src, const svthip_inter_planes* pred, const svthip_md_fast_desc* d_fast,
                                         const svthip_md_full_desc* d_full, uint32_t n_cand, const svthip_md_fast_group* d_group,
                                         const svthip_md_fast_pick* d_pick, uint32_t n_groups, uint32_t bwidth, uint32_t bheight, const int16_t* d_qparams,
                                         const int16_t* d_iscan, const uint32_t iscan_offsets[19 * 16], const svthip_coeff_rate_tables* d_tables,
                                         int32_t reduced_tx_set, uint32_t max_full, const svthip_inter_planes* slot_recon, uint32_t tiles_per_row,
                                         const svthip_inter_planes* recon, void* d_work, uint32_t stages, svthip_md_full_result* d_result,
                                         svthip_md_full128_tu* d_tu, svthip_md_full_decision* d_decision, void* stream)
{
    return md_full_loop(true, ctx, src, pred, d_fast, d_full, n_cand, d_group, d_pick, n_groups, bwidth, bheight, d_qparams, d_iscan, iscan_offsets, d_tables,
                        reduced_tx_set, 1, 1, max_full, slot_recon, tiles_per_row, recon, d_work, stages, d_result, d_tu, d_decision, stream);
}

// ---------------------------------------------------------------- mode decision's partition decision

uint32_t svthip_md_partition_geometry(uint32_t sb_size, svthip_md_partition_block* out, uint32_t max) { return svthip::md_part_geometry(sb_size, out, max); }

int32_t svthip_md_partition_batch_dev(svthip_ctx* ctx, const svthip_md_partition_sb* d_sb, uint32_t n_sb, const svthip_md_partition_leaf* d_leaf,
                                      uint32_t n_leaf, const svthip_md_full_decision* d_decision, uint32_t n_decision, uint32_t sb_size,
                                      int32_t slice_is_intra, const int32_t partition_fac_bits[20 * 11], svthip_md_partition_result* d_result,
                                      svthip_md_partition_final* d_final, uint32_t* d_final_count, void* stream)
{
    svthip::MdPartCall C = {};
    C.sb = d_sb, C.leaf = d_leaf, C.decision = d_decision, C.n_sb = n_sb, C.n_leaf = n_leaf, C.n_decision = n_decision, C.sb_size = sb_size;
    C.slice_is_intra = slice_is_intra, C.partition_fac_bits = partition_fac_bits, C.result = d_result, C.final_ = d_final, C.final_count = d_final_count;
    return md_partition(true, false, ctx, C, nullptr, nullptr, stream);
}

int32_t svthip_md_partition_compose_dev(svthip_ctx* ctx, uint32_t n_sb, const svthip_md_partition_leaf* d_leaf, uint32_t n_leaf, uint32_t sb_size,
                                        const svthip_md_partition_final* d_final, const uint32_t* d_final_count, const svthip_inter_planes* pool,
                                        uint32_t pool_width, uint32_t pool_height, const svthip_inter_planes* dst, uint32_t width, uint32_t height,
                                        void* stream)
{
    svthip::MdPartCall C = {};
    C.leaf = d_leaf, C.n_sb = n_sb, C.n_leaf = n_leaf, C.sb_size = sb_size;
    C.final_ = const_cast<svthip_md_partition_final*>(d_final), C.final_count = const_cast<uint32_t*>(d_final_count);
    C.pool_width = pool_width, C.pool_height = pool_height, C.width = width, C.height = height;
    return md_partition(false, true, ctx, C, pool, dst, stream);
}

int32_t svthip_md_partition_picture_dev(svthip_ctx* ctx, const svthip_md_partition_sb* d_sb, uint32_t n_sb, const svthip_md_partition_leaf* d_leaf,
                                        uint32_t n_leaf, const svthip_md_full_decision* d_decision, uint32_t n_decision, uint32_t sb_size,
                                        int32_t slice_is_intra, const int32_t partition_fac_bits[20 * 11], svthip_md_partition_result* d_result,
                                        svthip_md_partition_final* d_final, uint32_t* d_final_count, const svthip_inter_planes* pool,
                                        uint32_t pool_width, uint32_t pool_height, const svthip_inter_planes* dst, uint32_t width, uint32_t height,
                                        void* stream)
{
    svthip::MdPartCall C = {};
    C.sb = d_sb, C.leaf = d_leaf, C.decision = d_decision, C.n_sb = n_sb, C.n_leaf = n_leaf, C.n_decision = n_decision, C.sb_size = sb_size;
    C.slice_is_intra = slice_is_intra, C.partition_fac_bits = partition_fac_bits, C.result = d_result, C.final_ = d_final, C.final_count = d_final_count;
    C.pool_width = pool_width, C.pool_height = pool_height, C.width = width, C.height = height;
    return md_partition(true, true, ctx, C, pool, dst, stream);
}

}  // extern "C"
