// svt-av1-1_amd/csrc/md_full_kernels.h
//
// Mode decision's full loop on the device, gfx950: the kernels of md_full.hip and the arithmetic they share with the host test
// (tests/host_kernels/md_full_host.cpp compiles this header with g++ and calls the __device__ functions below on plain arrays).
// Replaces (paths under Source/Lib/Codec of the reference) what AV1PerformFullLoop (EbProductCodingLoop.c:2004-2307) does around the
// transform / quantisation chain and the coefficient rate, which stay the kernels of tq_encode_tu.hip and tq_coeff_rate.hip:
//   the candidate of a full-loop iteration, best_candidate_index_array                EbProductCodingLoop.c:2043-2054, :2573
//   the TU geometry of ProductFullLoop, ProductFullLoopTxSearch, FullLoop_R           EbFullLoop.c:946-1092, :1138-1351, :1763-1920
//   Av1TuCalcCostLuma with CBF_ZERO_OFF, Av1TuCalcCost's has_coeff bits               EbRateDistortionCost.c:2152-2230, :2051-2145
//   Av1FullCost, Av1MergeSkipFullCost                                                 EbRateDistortionCost.c:1485-1563, :1580-1721
//   the loop of product_full_mode_decision                                            EbModeDecision.c:1989-2012
//   the copy arm of AV1PerformInverseTransformRecon                                   EbProductCodingLoop.c:885-1038
//
//   expand    md_full_expand_luma_kernel / _chroma_kernel: a thread per slot (group, i) turns the pick into the slot's state and the
//             svthip_tu_desc / svthip_coeff_rate_desc rows of its TUs; with a tx-type search also one row per TxType of the masks' union
//             and the tx_search_tu_dev record of launch_tx_decision.  An inactive slot repeats a valid row, so every launch has the
//             shape the call's arguments give.
//   winner    md_full_luma_winner_kernel (search only): a thread per slot takes the decision's winner: its sums and bits become the
//             slot's, its TxType goes into the slot's TU descriptor for the launch that leaves levels and reconstruction.
//   cost      md_full_cost_kernel: a thread per slot, 64-bit integer arithmetic on a dozen loaded values per TU.
//   decide    md_full_decide_kernel: a thread per group over at most 12 result rows.
//   copy      md_full_copy_kernel: a thread per quad (four samples of a row) of the winner's Y, Cb and Cr blocks; a quad is one dword
//             load / store when its address is a multiple of 4, four byte accesses otherwise; no byte outside the block.
//
// A slot has 1 << (tu_log2_cols + tu_log2_rows) luma TUs of bw x bh side by side and as many TUs of cw x ch in Cb and in Cr: one for the 19
// block sizes with both sides <= 64, 2 or 4 TUs of 64x64 (chroma 32x32) for 128x64, 64x128 and 128x128 (txb_count of EbUtility.c:781-817;
// the loops over txb_itr of ProductFullLoop, FullLoop_R and CuFullDistortionFastTuMode_R, EbFullLoop.c:968-1091, :1801-1918, :1965-2082).
// Everything a launch of the chain or the rate reads or writes per TU is indexed by slot * TUs + TU, so all TUs of a plane are one launch.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svtav1_hip.h"
#define SVTHIP_MD_FAST_NO_KERNELS
#include "md_fast_kernels.h"   // md_fast_group_valid, md_fast_load_quad
#undef SVTHIP_MD_FAST_NO_KERNELS
#include "tq_tx_search_tu.h"

namespace svthip {

static_assert(sizeof(svthip_md_full_desc) == 48 && sizeof(svthip_md_full_result) == 144 && sizeof(svthip_md_full_decision) == 16 &&
                  sizeof(svthip_md_full128_tu) == 32 && sizeof(svthip_tu_desc) == 32 && sizeof(svthip_coeff_rate_desc) == 16 && sizeof(tx_search_tu_dev) == 80,
              "the layouts of include/svtav1_hip.h");

constexpr uint32_t MD_FULL_NONE = 0xffffffffu;   // no candidate row
constexpr uint64_t MD_FULL_MAX_COST = ~0ull;
constexpr int MD_FULL_THREADS = 64;              // per-slot and per-group kernels: little work a thread, many slots

// what a slot keeps between the stages (in the caller's workspace)
struct MdFullSlot {
    uint32_t row;       // the candidate's row, MD_FULL_NONE for an inactive slot
    uint32_t use_row;   // the row whose descriptors the slot's launches read: row, or a valid one repeated
    uint8_t tx_type_y, tx_type_uv;
    uint8_t bad_type;   // a TxType the chain has no network for: the slot ran as DCT_DCT and cannot win
    uint8_t reserved[5];
};
static_assert(sizeof(MdFullSlot) == 16, "one 16-byte store");

// ------------------------------------------------------------------------------------------------ geometry

// the 19 AV1 block sizes with both sides <= 64 are the 19 TxSizes: TxSize of (w, h), -1 for anything else (EbDefinitions.h:1178-1219)
__host__ __device__ __forceinline__ int md_full_tx_size(uint32_t w, uint32_t h)
{
    const int lw = w == 4 ? 0 : w == 8 ? 1 : w == 16 ? 2 : w == 32 ? 3 : w == 64 ? 4 : -1;
    const int lh = h == 4 ? 0 : h == 8 ? 1 : h == 16 ? 2 : h == 32 ? 3 : h == 64 ? 4 : -1;
    if (lw < 0 || lh < 0) return -1;
    if (lw == lh) return lw;                                    // TX_4X4 .. TX_64X64
    if (lh == lw + 1) return 5 + 2 * lw;                        // TX_4X8, TX_8X16, TX_16X32, TX_32X64
    if (lw == lh + 1) return 6 + 2 * lh;                        // TX_8X4, TX_16X8, TX_32X16, TX_64X32
    if (lh == lw + 2) return 13 + 2 * lw;                       // TX_4X16, TX_8X32, TX_16X64
    if (lw == lh + 2) return 14 + 2 * lh;                       // TX_16X4, TX_32X8, TX_64X16
    return -1;
}

// (MAX_TX_SCALE - av1_get_tx_scale) * 2 of a w x h transform (EbFullLoop.c:1043, EbTransforms.h:312-316)
__host__ __device__ __forceinline__ int md_full_dist_shift(uint32_t w, uint32_t h)
{
    const uint32_t pels = w * h;
    return (1 - ((pels > 256u) + (pels > 1024u))) * 2;
}

// the 1-D networks the chain has: ADST up to 16 points, identity up to 32 (fwd_txfm2d_type_valid of tq_fwd_txfm.hip)
__host__ __device__ __forceinline__ bool md_full_type_valid(uint32_t w, uint32_t h, uint32_t tx_type)
{
    if (tx_type > 15u) return false;
    const uint32_t vtx = 0xedce6244u, htx = 0xb73da850u;   // vtx_tab / htx_tab (EbTransforms.h:88-97), two bits a type: 0 DCT, 1 ADST, 2 FLIPADST, 3 IDTX
    const uint32_t kc = (vtx >> (2u * tx_type)) & 3u, kr = (htx >> (2u * tx_type)) & 3u;
    if ((kc == 1u || kc == 2u) && h > 16u) return false;
    if ((kr == 1u || kr == 2u) && w > 16u) return false;
    if (kc == 3u && h > 32u) return false;
    if (kr == 3u && w > 32u) return false;
    return true;
}

// RDCOST (EbRateDistortionCost.h:215-217) in the reference's unsigned 64-bit arithmetic
__host__ __device__ __forceinline__ uint64_t md_full_rdcost(uint64_t lambda, uint64_t rate, uint64_t dist) { return ((rate * lambda + 256u) >> 9) + (dist << 7); }

// RIGHT_SIGNED_SHIFT
__host__ __device__ __forceinline__ uint64_t md_full_shift(uint64_t v, int shift) { return shift < 0 ? v << -shift : v >> shift; }

// one call: the caller's arrays, the arrays in its workspace, the geometry
struct MdFullArgs {
    const svthip_md_fast_desc* fast;     // [n_cand]
    const svthip_md_full_desc* full;     // [n_cand]
    const svthip_md_fast_group* group;   // [n_groups]
    const svthip_md_fast_pick* pick;     // [n_groups]
    uint32_t n_cand, n_groups, max_full, n_slots;
    uint32_t src_stride[2], pred_stride[2], slot_stride[2], recon_stride[2];   // [0] Y, [1] Cb and Cr
    const uint8_t* slot_plane[3];
    uint8_t* recon_plane[3];
    uint32_t bw, bh, cw, ch;             // the luma TU and the TU of Cb / Cr
    uint32_t tu_log2_cols, tu_log2_rows; // the TUs of a slot side by side: 0, 0 for one TU (the block is the TU), 1 for two of 64 in that direction
    uint32_t tile_w, tile_h, tiles_per_row;
    uint32_t ncoef[2];                   // packed coefficients of a luma / chroma TU
    int tx_size_y, shift_y, shift_uv;
    uint32_t mask_inter, mask_intra;     // the types a slot's decision reads
    uint32_t n_types;                    // TxTypes of the masks' union; 0: no search
    uint8_t types[16];                   // ascending
    uint32_t iscan_y[16], iscan_uv[16];  // iscan_offsets of the two TxSizes
    uint8_t reduced_tx_set;
    // per slot (slots) and per (slot, TU) at slot * TUs + TU, in the workspace
    MdFullSlot* slots;
    svthip_tu_desc* tu[3];
    svthip_coeff_rate_desc* rate[3];
    uint16_t* eob[3];
    uint64_t* energy_y;
    uint64_t* dist[3];
    uint32_t* bits[3];
    const int32_t* qcoeff[3];
    // per (TxType of the union, slot), in the workspace: candidate j * n_slots + k
    svthip_tu_desc* s_tu;
    svthip_coeff_rate_desc* s_rate;
    tx_search_tu_dev* s_tus;             // [n_slots]
    uint32_t* s_bases;                   // [19 * 16]
    const uint64_t* s_energy;
    const uint64_t* s_dist;
    const uint32_t* s_bits;
    const svthip_tx_search_result* s_out;   // [n_slots]
    svthip_md_full_result* result;       // [n_slots]
    svthip_md_full128_tu* tu_out;        // [n_slots], null where the entry has none
    svthip_md_full_decision* decision;   // [n_groups]
    uint32_t* refused;
};

// TUs of a slot, and the luma offset of TU t inside the block (tx_org_x / tx_org_y of EbUtility.c:781-817)
__host__ __device__ __forceinline__ uint32_t md_full_tus(const MdFullArgs& A) { return 1u << (A.tu_log2_cols + A.tu_log2_rows); }
__host__ __device__ __forceinline__ uint32_t md_full_tu_x(const MdFullArgs& A, uint32_t t) { return (t & ((1u << A.tu_log2_cols) - 1u)) * A.bw; }
__host__ __device__ __forceinline__ uint32_t md_full_tu_y(const MdFullArgs& A, uint32_t t) { return (t >> A.tu_log2_cols) * A.bh; }

// ------------------------------------------------------------------------------------------------ expand

// the active slot count of a group (:2573), 0 for a group the pick refused
__device__ __forceinline__ uint32_t md_full_group_slots(const MdFullArgs& A, uint32_t g)
{
    const svthip_md_fast_group grp = A.group[g];
    const uint32_t full_count = A.pick[g].full_count;
    if (!md_fast_group_valid(grp, A.n_cand) || full_count == 0u) return 0u;
    const uint32_t n = min(full_count, min((uint32_t)grp.count, (uint32_t)grp.buffer_total_count));
    return min(n, A.max_full);
}

// the row of the candidate slot i of group g points at, MD_FULL_NONE for a buffer no candidate was written into
__device__ __forceinline__ uint32_t md_full_slot_row(const MdFullArgs& A, uint32_t g, uint32_t i)
{
    const uint32_t b = A.pick[g].best[i];
    if (b >= (uint32_t)MD_FAST_BUFFERS) return MD_FULL_NONE;
    const uint32_t c = A.pick[g].buffer_cand[b];
    return c < A.group[g].count ? A.group[g].first + c : MD_FULL_NONE;
}

// the luma position of slot k's tile in the slot planes
__device__ __forceinline__ void md_full_tile(const MdFullArgs& A, uint32_t k, uint32_t* x, uint32_t* y)
{
    *x = (k % A.tiles_per_row) * A.tile_w, *y = (k / A.tiles_per_row) * A.tile_h;
}

// plane 0: the luma TU at (x, y); planes 1, 2: the chroma TU at ((x >> 3) << 3) / 2
__device__ __forceinline__ uint32_t md_full_offset(uint32_t x, uint32_t y, uint32_t stride, int plane)
{
    return plane ? ((y >> 3) << 2) * stride + ((x >> 3) << 2) : y * stride + x;
}

// the TU and rate descriptors of TU tu of plane `plane` of slot k with TxType tx_type, reconstructing into its slot tile; every TU of a
// block has the block's contexts (EbRateDistortionCost.c:1377-1382)
__device__ __forceinline__ void md_full_emit_tu(const MdFullArgs& A, uint32_t k, uint32_t tu, uint32_t use_row, int plane, uint32_t tx_type)
{
    const svthip_md_fast_desc* f = A.fast + use_row;
    const svthip_md_full_desc* d = A.full + use_row;
    const int c = plane ? 1 : 0;
    const uint32_t j = k * md_full_tus(A) + tu, ox = md_full_tu_x(A, tu), oy = md_full_tu_y(A, tu);
    uint32_t tx, ty;
    md_full_tile(A, k, &tx, &ty);
    svthip_tu_desc t;
    t.src_offset = md_full_offset(f->src_x + ox, f->src_y + oy, A.src_stride[c], plane);
    t.pred_offset = md_full_offset(f->pred_x + ox, f->pred_y + oy, A.pred_stride[c], plane);
    t.recon_offset = md_full_offset(tx + ox, ty + oy, A.slot_stride[c], plane);
    t.coeff_offset = j * A.ncoef[c];
    t.iscan_offset = plane ? A.iscan_uv[tx_type] : A.iscan_y[tx_type];
    t.src_stride = (uint16_t)A.src_stride[c], t.pred_stride = (uint16_t)A.pred_stride[c], t.recon_stride = (uint16_t)A.slot_stride[c];
    t.qparam_index = d->qparam_index[plane];
    t.tx_type = (uint8_t)tx_type;
    t.reserved[0] = t.reserved[1] = t.reserved[2] = 0;
    A.tu[plane][j] = t;
    svthip_coeff_rate_desc r;
    r.coeff_offset = t.coeff_offset, r.iscan_offset = t.iscan_offset;
    r.tx_type = (uint8_t)tx_type, r.plane_type = (uint8_t)c;
    r.txb_skip_ctx = d->txb_skip_ctx[plane], r.dc_sign_ctx = d->dc_sign_ctx[plane];
    r.is_inter = (f->flags & SVTHIP_MD_FAST_TYPE_INTER) ? 1 : 0;
    r.intra_mode = d->intra_mode, r.reduced_tx_set = A.reduced_tx_set, r.reserved = 0;
    A.rate[plane][j] = r;
}

// Stage LUMA, slot k: its state and its luma descriptors.  Returns what the context counts: 1 for slot 0 of a group the pick refused,
// 1 for an active slot with a TxType the chain has no network for.
__device__ __forceinline__ uint32_t md_full_expand_luma(const MdFullArgs& A, uint32_t k)
{
    const uint32_t g = k / A.max_full, i = k % A.max_full;
    const uint32_t n_full = md_full_group_slots(A, g);
    const uint32_t row = i < n_full ? md_full_slot_row(A, g, i) : MD_FULL_NONE;
    uint32_t use_row = row;
    if (use_row == MD_FULL_NONE && n_full) use_row = md_full_slot_row(A, g, 0);
    if (use_row == MD_FULL_NONE) use_row = 0;
    uint32_t counted = (n_full == 0u && i == 0u) ? 1u : 0u;

    const svthip_md_full_desc* d = A.full + use_row;
    const bool is_inter = (A.fast[use_row].flags & SVTHIP_MD_FAST_TYPE_INTER) != 0;
    MdFullSlot s;
    s.row = row, s.use_row = use_row;
    s.tx_type_y = d->tx_type_y, s.tx_type_uv = d->tx_type_uv;
    if (A.n_types) s.tx_type_y = 0;                   // until the winner is known,
    if (A.n_types && is_inter) s.tx_type_uv = 0;      // which is an INTER slot's chroma type too
    s.bad_type = (uint8_t)(!md_full_type_valid(A.cw, A.ch, s.tx_type_uv) || !md_full_type_valid(A.bw, A.bh, s.tx_type_y));
    if (s.bad_type) s.tx_type_y = s.tx_type_uv = 0, counted += row != MD_FULL_NONE;
    s.reserved[0] = s.reserved[1] = s.reserved[2] = s.reserved[3] = s.reserved[4] = 0;
    A.slots[k] = s;
    for (uint32_t t = 0; t < md_full_tus(A); t++) md_full_emit_tu(A, k, t, use_row, 0, s.tx_type_y);

    if (A.n_types) {
        // the search (one TU a slot: the reference runs none from 128 on, EbProductCodingLoop.c:2133): one candidate per TxType of the
        // union, each with its own tile of bw x bh and its own levels
        const svthip_tu_desc base = A.tu[0][k];
        const svthip_coeff_rate_desc rbase = A.rate[0][k];
        const uint32_t mask = rbase.is_inter ? A.mask_inter : A.mask_intra;
        tx_search_tu_dev* tu = A.s_tus + k;
        tu->lambda = d->lambda, tu->tx_size = (uint32_t)A.tx_size_y, tu->reserved = 0;
        for (uint32_t t = 0; t < 16u; t++) tu->index[t] = ((mask >> t) & 1u) ? k : MD_FULL_NONE;
        for (uint32_t j = 0; j < A.n_types; j++) {
            const uint32_t pos = j * A.n_slots + k, t = A.types[j];
            svthip_tu_desc c = base;
            c.recon_offset = pos * (A.bw * A.bh), c.recon_stride = (uint16_t)A.bw;
            c.coeff_offset = pos * A.ncoef[0], c.iscan_offset = A.iscan_y[t], c.tx_type = (uint8_t)t;
            A.s_tu[pos] = c;
            svthip_coeff_rate_desc r = rbase;
            r.coeff_offset = c.coeff_offset, r.iscan_offset = c.iscan_offset, r.tx_type = (uint8_t)t;
            A.s_rate[pos] = r;
        }
        if (k == 0u) {   // where the run of every (TxSize, TxType) starts in the launch order: TxType types[j] of the luma TxSize at j * n_slots
            for (uint32_t e = 0; e < 19u * 16u; e++) A.s_bases[e] = 0;
            for (uint32_t j = 0; j < A.n_types; j++) A.s_bases[(uint32_t)A.tx_size_y * 16u + A.types[j]] = j * A.n_slots;
        }
    }
    return counted;
}

// Stage LUMA behind the decision of a search (one TU a slot), slot k: the winner's sums and bits become the slot's, its TxType the slot's
__device__ __forceinline__ void md_full_luma_winner(const MdFullArgs& A, uint32_t k)
{
    const uint32_t pos = A.s_out[k].candidate, t = A.s_out[k].tx_type;
    A.dist[0][2u * k] = A.s_dist[2u * (size_t)pos], A.dist[0][2u * k + 1u] = A.s_dist[2u * (size_t)pos + 1u];
    A.energy_y[k] = A.s_energy[pos];
    A.bits[0][k] = A.s_bits[pos];
    A.slots[k].tx_type_y = (uint8_t)t;
    if (A.rate[0][k].is_inter) A.slots[k].tx_type_uv = (uint8_t)t;   // TX_TYPE_FIX (EbFullLoop.c:1345-1347)
    A.tu[0][k].tx_type = A.rate[0][k].tx_type = (uint8_t)t, A.tu[0][k].iscan_offset = A.rate[0][k].iscan_offset = A.iscan_y[t];
}

// Stage CHROMA, slot k: the descriptors of its Cb and Cr TUs
__device__ __forceinline__ void md_full_expand_chroma(const MdFullArgs& A, uint32_t k)
{
    const MdFullSlot s = A.slots[k];
    for (uint32_t t = 0; t < md_full_tus(A); t++) {
        md_full_emit_tu(A, k, t, s.use_row, 1, s.tx_type_uv);
        md_full_emit_tu(A, k, t, s.use_row, 2, s.tx_type_uv);
    }
}

// ------------------------------------------------------------------------------------------------ cost

// what the walk over a slot's TUs of one plane, in the order of txb_itr, leaves: bits and distortions summed, bit t of the has_coeff mask
// TU t's, the last TU's first level (every TU overwrites quantized_dc), TU 0's eob
struct MdFullPlaneSums {
    uint64_t dist0, dist1, bits;   // DIST_CALC_RESIDUAL, DIST_CALC_PREDICTION
    int32_t quantized_dc;
    uint16_t eob;
    uint8_t has_coeff;
};

// Plane `plane` of slot k.  Luma: ProductFullLoop (EbFullLoop.c:968-1091) with Av1TuCalcCostLuma per TU, three_quad_energy the TU's own;
// chroma: CuFullDistortionFastTuMode_R (:1965-2082), no energy.  eob_out: the plane's row of the per-TU record.  The loop is unrolled to
// MAX_TU, the most TUs a slot of the call can have (1 or 4), and nothing is stored inside it, so that the loads of all TUs and planes of a
// slot are in flight together; with MAX_TU == 1 the walk is the straight line it was before there were slots of several TUs.
template <uint32_t MAX_TU>
__device__ __forceinline__ MdFullPlaneSums md_full_plane_sums(const MdFullArgs& A, uint32_t k, int plane, uint64_t lambda, uint16_t eob_out[4])
{
    MdFullPlaneSums o = {0, 0, 0, 0, 0, 0};
    const uint32_t n_tu = MAX_TU == 1u ? 1u : md_full_tus(A);
    const int shift = plane ? A.shift_uv : A.shift_y;
#pragma unroll
    for (uint32_t t = 0; t < MAX_TU; t++) {
        if (t >= n_tu) break;
        const uint32_t j = k * n_tu + t;
        const uint64_t energy = plane ? 0 : A.energy_y[j];
        uint64_t t0 = md_full_shift(A.dist[plane][2u * j] + energy, shift);
        const uint64_t t1 = md_full_shift(A.dist[plane][2u * j + 1u] + energy, shift);
        uint64_t t_bits = A.bits[plane][j];
        if (plane == 0 && !(md_full_rdcost(lambda, t_bits, t0) < MD_FULL_MAX_COST)) t_bits = 0, t0 = t1;   // against yZeroCbfCost = ~0
        o.dist0 += t0, o.dist1 += t1, o.bits += t_bits;
        const uint16_t eob = A.eob[plane][j];
        if (t == 0u) o.eob = eob;
        eob_out[t] = eob;
        o.has_coeff |= (uint8_t)((eob != 0) << t);
        o.quantized_dc = A.qcoeff[plane][(size_t)j * A.ncoef[plane ? 1 : 0]];
    }
    return o;
}

// Stage DECIDE, slot k: its result row and its per-TU record (all 0 for a slot without a cost; stored only where the entry has one)
template <uint32_t MAX_TU>
__device__ __forceinline__ svthip_md_full_result md_full_cost(const MdFullArgs& A, uint32_t k, svthip_md_full128_tu* tu_out)
{
    const MdFullSlot s = A.slots[k];
    svthip_md_full_result r;
    memset(&r, 0, sizeof(r));
    memset(tu_out, 0, sizeof(*tu_out));
    r.row = s.row, r.tx_type_y = s.tx_type_y, r.tx_type_uv = s.tx_type_uv;
    r.full_cost = MD_FULL_MAX_COST;
    if (s.row == MD_FULL_NONE) return r;
    const svthip_md_fast_desc* f = A.fast + s.row;
    const svthip_md_full_desc* d = A.full + s.row;
    if ((f->flags & SVTHIP_MD_FAST_INVALID) || s.bad_type) return r;
    const uint64_t lambda = d->lambda;

    const MdFullPlaneSums y = md_full_plane_sums<MAX_TU>(A, k, 0, lambda, tu_out->eob[0]);
    const uint64_t y0 = y.dist0, y1 = y.dist1, y_bits = y.bits;
    uint64_t uv0 = 0, uv1 = 0;   // Cb + Cr
    r.y_distortion[0] = y0, r.y_distortion[1] = y1;
    r.coeff_bits[0] = y_bits, r.eob[0] = y.eob, r.quantized_dc[0] = y.quantized_dc, r.y_has_coeff = y.has_coeff;
    if (f->has_uv) {
        const MdFullPlaneSums cb = md_full_plane_sums<MAX_TU>(A, k, 1, lambda, tu_out->eob[1]);
        const MdFullPlaneSums cr = md_full_plane_sums<MAX_TU>(A, k, 2, lambda, tu_out->eob[2]);
        r.cb_distortion[0] = cb.dist0, r.cb_distortion[1] = cb.dist1, r.cr_distortion[0] = cr.dist0, r.cr_distortion[1] = cr.dist1;
        r.coeff_bits[1] = cb.bits, r.coeff_bits[2] = cr.bits, r.eob[1] = cb.eob, r.eob[2] = cr.eob;
        uv0 = cb.dist0 + cr.dist0, uv1 = cb.dist1 + cr.dist1;
        r.quantized_dc[1] = cb.quantized_dc, r.quantized_dc[2] = cr.quantized_dc, r.u_has_coeff = cb.has_coeff, r.v_has_coeff = cr.has_coeff;
    }
    r.block_has_coeff = (r.y_has_coeff | r.u_has_coeff | r.v_has_coeff) != 0;

    const uint64_t coeff_rate = r.coeff_bits[0] + r.coeff_bits[1] + r.coeff_bits[2];
    const uint64_t rate = (uint64_t)d->luma_rate + d->chroma_rate + coeff_rate;
    const uint64_t distortion = y0 + uv0;
    // the numbers of the two arms as scalars, stored once: stores into r from inside the arms keep part of r in scratch
    const bool merge = d->skip_mode_rate != 0xffffffffu;
    const uint64_t skip_distortion = y1 + uv1;
    const uint64_t full = md_full_rdcost(lambda, rate, distortion);                                   // Av1FullCost, and the merge arm's merge cost
    const uint64_t skip = md_full_rdcost(lambda, merge ? d->skip_mode_rate : 0u, skip_distortion);   // Av1MergeSkipFullCost
    const bool skip_flag = merge && skip <= full;
    r.merge_cost = merge ? full : 0, r.skip_cost = merge ? skip : 0, r.skip_flag = skip_flag;
    r.full_cost = skip_flag ? skip : full;
    r.full_lambda_rate = skip_flag ? skip - skip_distortion : full - distortion;
    r.full_cost_luma = merge ? 0 : md_full_rdcost(lambda, (uint64_t)d->luma_rate + y_bits, y0);
    return r;
}

// the row alone, for any TU count
__device__ __forceinline__ svthip_md_full_result md_full_cost(const MdFullArgs& A, uint32_t k)
{
    svthip_md_full128_tu unused;
    return md_full_cost<4>(A, k, &unused);
}

// ------------------------------------------------------------------------------------------------ decision

// Stage DECIDE, group g: product_full_mode_decision's loop over the group's result rows
__device__ __forceinline__ svthip_md_full_decision md_full_decide(const MdFullArgs& A, uint32_t g)
{
    svthip_md_full_decision o;
    const uint32_t n_full = md_full_group_slots(A, g);
    o.cost = MD_FULL_MAX_COST, o.winner_row = MD_FULL_NONE;
    o.winner_slot = o.winner_buffer = o.best_intra_mode = 0xff, o.n_full = (uint8_t)n_full;
    if (n_full == 0u) return o;
    const svthip_md_full_result* rows = A.result + (size_t)g * A.max_full;
    uint64_t lowest = MD_FULL_MAX_COST, lowest_intra = MD_FULL_MAX_COST;
    uint32_t win = 0;
    for (uint32_t i = 0; i < n_full; i++) {
        const uint64_t cost = rows[i].full_cost;
        const uint32_t row = rows[i].row;
        if (cost < lowest_intra && row != MD_FULL_NONE && !(A.fast[row].flags & SVTHIP_MD_FAST_TYPE_INTER))
            o.best_intra_mode = A.full[row].intra_mode, lowest_intra = cost;
        if (cost < lowest) win = i, lowest = cost;
    }
    o.winner_slot = (uint8_t)win, o.winner_buffer = A.pick[g].best[win];
    o.winner_row = rows[win].row, o.cost = rows[win].full_cost;
    return o;
}

// ------------------------------------------------------------------------------------------------ copy

// quads of a group's blocks of bw x bh (Cb, Cr: cw x ch): Y, then Cb, then Cr
__host__ __device__ __forceinline__ uint32_t md_full_copy_quads(uint32_t bw, uint32_t bh, uint32_t cw, uint32_t ch) { return bw / 4u * bh + 2u * (cw / 4u * ch); }

__device__ __forceinline__ void md_full_store_quad(uint8_t* p, uint32_t v)
{
    if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
        *reinterpret_cast<uint32_t*>(p) = v;
#else
        memcpy(p, &v, 4);
#endif
        return;
    }
    p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}

// Stage DECIDE, quad q of group g: the winner's slot tile to its block of the reconstructed picture
__device__ __forceinline__ void md_full_copy_quad(const MdFullArgs& A, uint32_t g, uint32_t q)
{
    const svthip_md_full_decision dec = A.decision[g];
    if (dec.winner_row == MD_FULL_NONE) return;
    const uint32_t yw = A.bw << A.tu_log2_cols, yh = A.bh << A.tu_log2_rows, uvw = A.cw << A.tu_log2_cols, uvh = A.ch << A.tu_log2_rows;   // the block
    const uint32_t luma_quads = yw / 4u * yh, chroma_quads = uvw / 4u * uvh;
    int plane = 0;
    uint32_t qw = yw / 4u;
    if (q >= luma_quads) {
        if (!A.fast[dec.winner_row].has_uv) return;
        q -= luma_quads, plane = 1, qw = uvw / 4u;
        if (q >= chroma_quads) q -= chroma_quads, plane = 2;
    }
    const int c = plane ? 1 : 0;
    uint32_t tx, ty;
    md_full_tile(A, g * A.max_full + dec.winner_slot, &tx, &ty);
    const svthip_md_full_desc* d = A.full + dec.winner_row;
    const uint32_t r = q / qw, x = (q % qw) * 4u;
    const uint8_t* from = A.slot_plane[plane] + md_full_offset(tx, ty, A.slot_stride[c], plane) + (size_t)r * A.slot_stride[c] + x;
    uint8_t* to = A.recon_plane[plane] + md_full_offset(d->recon_x, d->recon_y, A.recon_stride[c], plane) + (size_t)r * A.recon_stride[c] + x;
    md_full_store_quad(to, md_fast_load_quad(from));
}

#ifdef __HIPCC__

// ------------------------------------------------------------------------------------------------ kernels

__global__ void __launch_bounds__(MD_FULL_THREADS) md_full_expand_luma_kernel(MdFullArgs A)
{
    const uint32_t k = blockIdx.x * MD_FULL_THREADS + threadIdx.x;
    if (k >= A.n_slots) return;
    const uint32_t counted = md_full_expand_luma(A, k);
    if (counted) atomicAdd(A.refused, counted);
}

__global__ void __launch_bounds__(MD_FULL_THREADS) md_full_luma_winner_kernel(MdFullArgs A)
{
    const uint32_t k = blockIdx.x * MD_FULL_THREADS + threadIdx.x;
    if (k < A.n_slots) md_full_luma_winner(A, k);
}

__global__ void __launch_bounds__(MD_FULL_THREADS) md_full_expand_chroma_kernel(MdFullArgs A)
{
    const uint32_t k = blockIdx.x * MD_FULL_THREADS + threadIdx.x;
    if (k < A.n_slots) md_full_expand_chroma(A, k);
}

template <uint32_t MAX_TU>
__global__ void __launch_bounds__(MD_FULL_THREADS) md_full_cost_kernel(MdFullArgs A)
{
    const uint32_t k = blockIdx.x * MD_FULL_THREADS + threadIdx.x;
    if (k >= A.n_slots) return;
    union {
        uint4 q[9];
        svthip_md_full_result r;
    } o;
    union {
        uint4 q[2];
        svthip_md_full128_tu t;
    } u;
    o.r = md_full_cost<MAX_TU>(A, k, &u.t);
    uint4* dst = reinterpret_cast<uint4*>(A.result + k);
#pragma unroll
    for (int w = 0; w < 9; w++) dst[w] = o.q[w];
    if (A.tu_out) {
        uint4* tdst = reinterpret_cast<uint4*>(A.tu_out + k);
        tdst[0] = u.q[0], tdst[1] = u.q[1];
    }
}

__global__ void __launch_bounds__(MD_FULL_THREADS) md_full_decide_kernel(MdFullArgs A)
{
    const uint32_t g = blockIdx.x * MD_FULL_THREADS + threadIdx.x;
    if (g >= A.n_groups) return;
    union {
        uint4 q;
        svthip_md_full_decision d;
    } o;
    o.d = md_full_decide(A, g);
    *reinterpret_cast<uint4*>(A.decision + g) = o.q;
}

__global__ void __launch_bounds__(256) md_full_copy_kernel(MdFullArgs A)
{
    const uint32_t per_group = md_full_copy_quads(A.bw << A.tu_log2_cols, A.bh << A.tu_log2_rows, A.cw << A.tu_log2_cols, A.ch << A.tu_log2_rows);
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)A.n_groups * per_group) return;
    md_full_copy_quad(A, (uint32_t)(t / per_group), (uint32_t)(t % per_group));
}

#endif  // __HIPCC__

}  // namespace svthip
