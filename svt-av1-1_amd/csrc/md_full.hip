// svt-av1-1_amd/csrc/md_full.hip
//
// Mode decision's full loop on the device, gfx950: the launches of md_full_kernels.h around the launch paths of the fused chain
// (tq_encode_tu.hip), the coefficient rate and the tx-type decision (tq_coeff_rate.hip).  Replaces AV1PerformFullLoop
// (Source/Lib/Codec/EbProductCodingLoop.c:2004-2307) and the loop of product_full_mode_decision (Codec/EbModeDecision.c:1989-2012) for the
// blocks of one luma size whose picks svthip_md_fast_pick_batch_dev left in device memory.  A call is: expand -> chain -> rate
// [-> decision -> winner -> chain] for luma, expand -> chain -> rate for Cb and for Cr, cost -> decide -> copy, all on one stream, every
// launch of a shape the call's arguments give.  The same launches serve the 128-wide blocks (svthip_md_full_loop128_batch_dev): their 2 or
// 4 TUs a slot (the loops over txb_itr of Codec/EbFullLoop.c:968-1091, :1801-1918, :1965-2082) are more descriptors of the one chain and
// the one rate launch of a plane, never more launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svtav1_hip.h"
#include "md_launch.h"
#include "tq_launch.h"
#include "md_full_kernels.h"

namespace svthip {

namespace {

size_t round16(size_t v) { return (v + 15u) & ~(size_t)15u; }

uint32_t blocks_of(uint64_t n, uint32_t threads) { return (uint32_t)((n + threads - 1u) / threads); }

template <typename T>
T* at(void* work, size_t offset) { return reinterpret_cast<T*>(static_cast<uint8_t*>(work) + offset); }

}  // namespace

bool md_full_size_ok(uint32_t bwidth, uint32_t bheight, bool wide)
{
    if (wide) return (bwidth == 128u && (bheight == 128u || bheight == 64u)) || (bwidth == 64u && bheight == 128u);
    return md_full_tx_size(bwidth, bheight) >= 0;
}

// The caller's workspace for n_groups * max_full slots of bw x bh: per slot its state, per (slot, TU) the descriptors, eobs, sums, bits
// and levels of the TU in Y, Cb and Cr; with a search (a mask with more than bit 0) per (TxType of the union, slot) the same for the luma
// candidates, their tiles, and per slot the record and the result of the decision.  False: arguments the entry refuses, or offsets beyond
// 32 bits.
bool md_full_layout(uint32_t n_groups, uint32_t max_full, uint32_t bw, uint32_t bh, bool wide, uint32_t mask_inter, uint32_t mask_intra, MdFullLayout* L)
{
    if (!md_full_size_ok(bw, bh, wide) || max_full < 1u || max_full > SVTHIP_MD_FULL_MAX_SLOTS) return false;
    if (!mask_inter || !mask_intra || ((mask_inter | mask_intra) >> 16)) return false;
    if (wide && (mask_inter | mask_intra) != 1u) return false;   // no search from 128 on (Codec/EbProductCodingLoop.c:2133)
    L->tu_log2_cols = bw > 64u, L->tu_log2_rows = bh > 64u;
    L->tu_w = bw >> L->tu_log2_cols, L->tu_h = bh >> L->tu_log2_rows;
    bw = L->tu_w, bh = L->tu_h;                                   // from here on the TU
    const uint32_t both = mask_inter | mask_intra;
    L->n_types = 0;
    for (uint32_t t = 0; t < 16u; t++)
        if ((both >> t) & 1u) {
            if (!md_full_type_valid(bw, bh, t)) return false;
            L->types[L->n_types++] = (uint8_t)t;
        }
    if (both == 1u) L->n_types = 0;   // DCT_DCT alone: no search
    const uint64_t slots = (uint64_t)n_groups * max_full, n = slots << (L->tu_log2_cols + L->tu_log2_rows), m = slots * L->n_types;
    const uint32_t cw = bw / 2u < 4u ? 4u : bw / 2u, ch = bh / 2u < 4u ? 4u : bh / 2u;
    const uint64_t ncoef_y = (uint64_t)(bw < 32u ? bw : 32u) * (bh < 32u ? bh : 32u), ncoef_uv = (uint64_t)cw * ch;
    if (n * ncoef_y > 0xffffffffull || m * ncoef_y > 0xffffffffull || m * bw * bh > 0xffffffffull) return false;
    L->n_slots = (uint32_t)slots;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t here = o; o += round16(bytes); return here; };
    L->slots = take(slots * sizeof(MdFullSlot));
    for (int p = 0; p < 3; p++) {
        const uint64_t ncoef = p ? ncoef_uv : ncoef_y;
        L->tu[p] = take(n * sizeof(svthip_tu_desc)), L->rate[p] = take(n * sizeof(svthip_coeff_rate_desc));
        L->eob[p] = take(n * sizeof(uint16_t)), L->dist[p] = take(n * 2u * sizeof(uint64_t)), L->bits[p] = take(n * sizeof(uint32_t));
        L->qcoeff[p] = take(n * ncoef * sizeof(int32_t));
    }
    L->energy_y = take(n * sizeof(uint64_t));
    L->s_tu = take(m * sizeof(svthip_tu_desc)), L->s_rate = take(m * sizeof(svthip_coeff_rate_desc));
    L->s_eob = take(m * sizeof(uint16_t)), L->s_energy = take(m * sizeof(uint64_t)), L->s_dist = take(m * 2u * sizeof(uint64_t));
    L->s_bits = take(m * sizeof(uint32_t)), L->s_qcoeff = take(m * ncoef_y * sizeof(int32_t)), L->s_recon = take(m * bw * bh);
    L->s_tus = take(L->n_types ? slots * sizeof(tx_search_tu_dev) : 0), L->s_bases = take(L->n_types ? 19u * 16u * sizeof(uint32_t) : 0);
    L->s_out = take(L->n_types ? slots * sizeof(svthip_tx_search_result) : 0);
    L->total = o;
    return true;
}

hipError_t launch_md_full_loop(const MdFullCall& C, const MdFullLayout& L, hipStream_t s)
{
    const uint32_t n = L.n_slots, m = n * L.n_types, n_tus = n << (L.tu_log2_cols + L.tu_log2_rows);   // slots, search candidates, TUs of a plane
    void* w = C.work;
    MdFullArgs A;
    A.fast = C.fast, A.full = C.full, A.group = C.group, A.pick = C.pick;
    A.n_cand = C.n_cand, A.n_groups = C.n_groups, A.max_full = C.max_full, A.n_slots = n;
    A.src_stride[0] = C.src.y_stride, A.src_stride[1] = C.src.c_stride, A.pred_stride[0] = C.pred.y_stride, A.pred_stride[1] = C.pred.c_stride;
    A.slot_stride[0] = C.slot_recon.y_stride, A.slot_stride[1] = C.slot_recon.c_stride;
    A.recon_stride[0] = C.recon.y_stride, A.recon_stride[1] = C.recon.c_stride;
    void* const src[3] = {C.src.y, C.src.cb, C.src.cr};
    void* const pred[3] = {C.pred.y, C.pred.cb, C.pred.cr};
    void* const slot[3] = {C.slot_recon.y, C.slot_recon.cb, C.slot_recon.cr};
    void* const recon[3] = {C.recon.y, C.recon.cb, C.recon.cr};
    for (int p = 0; p < 3; p++) A.slot_plane[p] = static_cast<const uint8_t*>(slot[p]), A.recon_plane[p] = static_cast<uint8_t*>(recon[p]);
    A.bw = L.tu_w, A.bh = L.tu_h, A.tu_log2_cols = L.tu_log2_cols, A.tu_log2_rows = L.tu_log2_rows;
    A.cw = A.bw / 2u < 4u ? 4u : A.bw / 2u, A.ch = A.bh / 2u < 4u ? 4u : A.bh / 2u;
    A.tile_w = C.bwidth < 8u ? 8u : C.bwidth, A.tile_h = C.bheight < 8u ? 8u : C.bheight, A.tiles_per_row = C.tiles_per_row;
    A.ncoef[0] = (A.bw < 32u ? A.bw : 32u) * (A.bh < 32u ? A.bh : 32u), A.ncoef[1] = A.cw * A.ch;
    A.tx_size_y = md_full_tx_size(A.bw, A.bh);
    const int tx_size_uv = md_full_tx_size(A.cw, A.ch);
    A.shift_y = md_full_dist_shift(A.bw, A.bh), A.shift_uv = md_full_dist_shift(A.cw, A.ch);
    A.mask_inter = C.type_mask_inter, A.mask_intra = C.type_mask_intra;
    A.n_types = L.n_types;
    for (int t = 0; t < 16; t++) {
        A.types[t] = L.types[t];
        A.iscan_y[t] = C.iscan_offsets[A.tx_size_y * 16 + t], A.iscan_uv[t] = C.iscan_offsets[tx_size_uv * 16 + t];
    }
    A.reduced_tx_set = C.reduced_tx_set ? 1 : 0;
    A.slots = at<MdFullSlot>(w, L.slots);
    int32_t* qcoeff[3];
    for (int p = 0; p < 3; p++) {
        A.tu[p] = at<svthip_tu_desc>(w, L.tu[p]), A.rate[p] = at<svthip_coeff_rate_desc>(w, L.rate[p]);
        A.eob[p] = at<uint16_t>(w, L.eob[p]), A.dist[p] = at<uint64_t>(w, L.dist[p]), A.bits[p] = at<uint32_t>(w, L.bits[p]);
        A.qcoeff[p] = qcoeff[p] = at<int32_t>(w, L.qcoeff[p]);
    }
    A.energy_y = at<uint64_t>(w, L.energy_y);
    A.s_tu = at<svthip_tu_desc>(w, L.s_tu), A.s_rate = at<svthip_coeff_rate_desc>(w, L.s_rate);
    A.s_tus = at<tx_search_tu_dev>(w, L.s_tus), A.s_bases = at<uint32_t>(w, L.s_bases);
    uint16_t* s_eob = at<uint16_t>(w, L.s_eob);
    uint64_t *s_energy = at<uint64_t>(w, L.s_energy), *s_dist = at<uint64_t>(w, L.s_dist);
    uint32_t* s_bits = at<uint32_t>(w, L.s_bits);
    svthip_tx_search_result* s_out = at<svthip_tx_search_result>(w, L.s_out);
    A.s_energy = s_energy, A.s_dist = s_dist, A.s_bits = s_bits, A.s_out = s_out;
    A.result = C.result, A.tu_out = C.tu_out, A.decision = C.decision, A.refused = C.refused;

    const dim3 per_slot(blocks_of(n, MD_FULL_THREADS)), threads(MD_FULL_THREADS);
    hipError_t e;
    auto chain = [&](int p, void* recon_plane, const svthip_tu_desc* desc, uint32_t count, int32_t* levels, uint16_t* eob, uint64_t* energy, uint64_t* dist) {
        return launch_encode_tu(src[p], pred[p], recon_plane, 0, desc, count, (int)(p ? A.cw : A.bw), (int)(p ? A.ch : A.bh), C.qparams, C.iscan, nullptr,
                                levels, nullptr, eob, energy, dist, C.max_workgroups, s);
    };
    auto rate = [&](int p, const int32_t* levels, const uint16_t* eob, const svthip_coeff_rate_desc* desc, uint32_t count, uint32_t* bits) {
        return launch_coeff_rate(C.tables, levels, eob, C.iscan, desc, count, p ? tx_size_uv : A.tx_size_y, bits, s);
    };

    if (C.stages & SVTHIP_MD_FULL_LUMA) {
        hipLaunchKernelGGL(md_full_expand_luma_kernel, per_slot, threads, 0, s, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (L.n_types) {
            if ((e = chain(0, at<uint8_t>(w, L.s_recon), A.s_tu, m, at<int32_t>(w, L.s_qcoeff), s_eob, s_energy, s_dist)) != hipSuccess) return e;
            if ((e = rate(0, at<int32_t>(w, L.s_qcoeff), s_eob, A.s_rate, m, s_bits)) != hipSuccess) return e;
            if ((e = launch_tx_decision(A.s_tus, n, A.s_bases, s_eob, s_energy, s_dist, s_bits, s_out, s)) != hipSuccess) return e;
            hipLaunchKernelGGL(md_full_luma_winner_kernel, per_slot, threads, 0, s, A);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            // the winner once more, as ProductFullLoop runs it: its levels, its eob, its reconstruction in the slot tile
            if ((e = chain(0, slot[0], A.tu[0], n, qcoeff[0], A.eob[0], nullptr, nullptr)) != hipSuccess) return e;
        } else {
            if ((e = chain(0, slot[0], A.tu[0], n_tus, qcoeff[0], A.eob[0], A.energy_y, A.dist[0])) != hipSuccess) return e;
            if ((e = rate(0, qcoeff[0], A.eob[0], A.rate[0], n_tus, A.bits[0])) != hipSuccess) return e;
        }
    }
    if (C.stages & SVTHIP_MD_FULL_CHROMA) {
        hipLaunchKernelGGL(md_full_expand_chroma_kernel, per_slot, threads, 0, s, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        for (int p = 1; p < 3; p++) {
            if ((e = chain(p, slot[p], A.tu[p], n_tus, qcoeff[p], A.eob[p], nullptr, A.dist[p])) != hipSuccess) return e;
            if ((e = rate(p, qcoeff[p], A.eob[p], A.rate[p], n_tus, A.bits[p])) != hipSuccess) return e;
        }
    }
    if (C.stages & SVTHIP_MD_FULL_DECIDE) {
        if (n_tus == n) hipLaunchKernelGGL(md_full_cost_kernel<1>, per_slot, threads, 0, s, A);   // one TU a slot: the walk as a straight line
        else hipLaunchKernelGGL(md_full_cost_kernel<4>, per_slot, threads, 0, s, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(md_full_decide_kernel, dim3(blocks_of(C.n_groups, MD_FULL_THREADS)), threads, 0, s, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(md_full_copy_kernel, dim3(blocks_of((uint64_t)C.n_groups * md_full_copy_quads(C.bwidth, C.bheight, A.cw << A.tu_log2_cols, A.ch << A.tu_log2_rows), 256u)), dim3(256), 0, s, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace svthip
