// svt-av1-1_amd/csrc/tq_encode_tu.hip
//
// Fused per-TU encode chain for 8-bit luma/chroma transform units, gfx950: one kernel does what Av1EncodeLoop
// (Source/Lib/Codec/EbCodingLoop.c:552-760) does per TU with five calls --
//   ResidualKernel (Codec/EbPictureOperators.c:257-285)            source - prediction
//   Av1EstimateTransform (Codec/EbTransforms.c:4410-4728)          forward 2-D transform, 64-point packing + three_quad_energy
//   Av1QuantizeInvQuantize (Codec/EbFullLoop.c:877-941)            quantise / dequantise / eob
//   FullDistortionKernel32Bits (Codec/EbPictureOperators.c:374-404) coefficient-domain distortion (mode decision's full loop)
//   Av1InvTransformRecon8bit (Codec/EbTransforms.c:8374-8399)      inverse transform + reconstruction
// -- with the residual, the coefficients and the dequantised coefficients never leaving registers / LDS.  HBM traffic per
// pixel: 1 B source + 1 B prediction + 2 B inverse-scan index in, 4 B quantised coefficient + 1 B reconstruction out
// (+ 4 B each for the optional transform / dequantised outputs), against 28 B for the five separate passes.
//
// Mapping (TxTile, tq_tile.h): a wave owns G = 64 / min(W, H) TUs, so the pass over the SHORTER dimension's lanes fills the wave exactly and the pass
// over the longer one takes max / min rounds of 64 lanes (with G = 64 / max the 4:1 rectangles ran one pass at 25 % of the lanes).
//   A  lane = (tu, column): residual column -> forward column network -> LDS tile
//   B  lane = (tu, row):    forward row network -> coefficients (registers) -> energy of the dropped part of 64-point
//                           dimensions, quantiser, distortion, eob (reductions across the TU's lanes) -> inverse row
//                           network on the dequantised row -> LDS tile (same row, same lane)
//   C  lane = (tu, column): inverse column network -> prediction + residual -> clip -> reconstruction
// Square sizes (round 3): the planes are touched by ROWS.  Read by columns, every sample was its own byte load -- a wave instruction
// that moves 64 bytes and costs the texture path as many tag look-ups as a 1 KB one; the counters of the column form showed 63 memory
// instructions and ~1440 L1 accesses per 1024 pixels with the L1 / data-return units ~90 % busy (profiles/r03_pmcx_tq_before.txt) while the
// vector unit idled a third of the time.  Now
//   A0 lane = (tu, row): source and prediction row in one wide load each -> residual row -> LDS tile (rows)
//   A  lane = (tu, column): column from the tile -> forward column network -> tile
//   B  as above
//   C  lane = (tu, column): inverse column network -> clamped residual -> tile
//   D  lane = (tu, row): residual row from the tile + the prediction row kept in registers since A0 -> clip -> one wide store
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svtav1_hip.h"
#include "tq_launch.h"
#include "tq_tile.h"

namespace svthip {

namespace {

#include "tq_txfm_common.h"
#include "tq_fwd_networks.h"
#include "tq_inv_networks.h"
#include "tq_quant_common.h"

// One row of a TU as N dwords at byte alignment (global_load_dword / x2 / x4; this target needs no alignment for them).
template <int N>
struct __attribute__((packed, aligned(1))) unaligned_row { uint32_t v[N]; };

// PIX = uint8_t: 8-bit planes (bd 8, quantize_b_helper_c_II); PIX = uint16_t: 10-bit samples in 16-bit planes (bd 10,
// highbd_quantize_b_helper_c, Av1InvTransformRecon)
// DIST: the coefficient-domain distortion sums of mode decision's full loop are wanted (dist_out != NULL).  The encode pass does not ask
// for them, and they cost three vector instructions per coefficient plus two 64-bit reductions per TU in a kernel that is bound by
// vector-instruction issue: a template parameter, not a run-time test inside the coefficient loop.
// 64-point sizes: their LDS tiles allow two waves per SIMD anyway, so the register allocator gets all 256 (left at its default it squeezed the
// variant without distortion sums into 165 VGPRs and that code ran 40 % slower than the 213-VGPR one).
template <int WL, int HL, typename PIX, bool DIST>
__global__ void __launch_bounds__(256, (WL >= 6 || HL >= 6) ? 2 : 1) encode_tu_kernel(const PIX* __restrict__ src, const PIX* pred,
                                                        PIX* recon, const svthip_tu_desc* __restrict__ desc, uint32_t n_tu,
                                                        const int16_t* __restrict__ qparams, const int16_t* __restrict__ iscan_pool,
                                                        int32_t* __restrict__ coeff_out, int32_t* __restrict__ qcoeff_out,
                                                        int32_t* __restrict__ dqcoeff_out, uint16_t* __restrict__ eob_out,
                                                        uint64_t* __restrict__ energy_out, uint64_t* __restrict__ dist_out)
{
    using T = TxTile<WL, HL>;
    constexpr int W = T::W, H = T::H, G = T::G, P = T::P, WIN = T::WIN, HIN = T::HIN;
    constexpr int SH0 = kShift[T::WI][T::HI][0], SH1 = kShift[T::WI][T::HI][1], SH2 = kShift[T::WI][T::HI][2];
    constexpr int BITC = kCosCol[T::WI][T::HI], BITR = kCosRow[T::WI][T::HI];
    constexpr int ISH0 = kInvShift0[T::WI][T::HI];
    constexpr int LOG_SCALE = (W * H > 256) + (W * H > 1024);  // av1_get_tx_scale (EbTransforms.h:312-316)
    extern __shared__ int32_t lds_all[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // QSTAGE (square sizes up to 32): the quantised coefficients leave through a per-wave LDS image [64 rows][W + 4] and are stored as
    // contiguous 1 KB pieces per instruction.  Stored straight from the row lanes, every lane's 16 bytes were their own write request at the L2
    // (64 per instruction, 256 per group of 1024 pixels), and the stamps showed the row pass -- the one that issues them -- taking half of a
    // group's time with a 4x spread (an earlier run of tools/tq_stamps_probe.py; profiles/r03_tq_stamps_16x16.txt is the current build): waves queueing at the vector-memory issue.
    constexpr bool QSTAGE = T::QSTAGE;
    constexpr int QP_ = T::QP;                                  // staging row pitch in dwords: 16-byte rows at a stride that spreads the banks
    int32_t* tile = lds_all + wave * (T::tile_words + T::stage_words);
    int32_t* qst = tile + T::tile_words;  // [64][QP_] then coeff_offset of the group's TUs [16]
    constexpr int BD = sizeof(PIX) == 1 ? 8 : 10, HIGHBD = sizeof(PIX) == 1 ? 0 : 1;
    const TxLimits lim = tx_limits(BD);
    const uint32_t groups = T::groups(n_tu);
    // Square sizes (one round per pass, the same TU on a lane in every pass): everything a group reads from memory is requested
    // AHEAD of the group, and the prediction row stays in registers (packed as loaded) for the reconstruction.  A wave walks its groups with
    // a two-step prefetch: the descriptor of the next group is requested at the top of the current one, the next group's source /
    // prediction rows, quantiser row and (sizes up to 16) inverse-scan row after the current group's column pass.  With one group per wave
    // and ~3.4 waves per SIMD the counters showed a wave issuing a quarter of its 27 k-cycle life -- descriptor, then rows, then the
    // stores, three exposed round trips -- and the vector unit busy 0.71 (profiles/r03_pmcx_tq_rows.txt).
    constexpr int PER = 4 / (int)sizeof(PIX), PBITS = 8 * (int)sizeof(PIX);  // samples per dword
    constexpr bool HOIST = T::template HOIST<PIX>, HOIST_ISCAN = T::template HOIST_ISCAN<PIX>;
    constexpr int ROWDW = HOIST ? W / PER : 1;
    constexpr bool PIPE = T::PIPE;  // 64x64 has no registers to spare for a second set of rows: it fetches at the top of each group
    const uint32_t gstride = gridDim.x * 4;
    const int hg = lane / W, hi = lane % W;  // square sizes: the lane's TU of the group and its row (A0, B, D) / column (A, C)
    svthip_tu_desc d_nx{};                   // next group: descriptor ...
    unaligned_row<ROWDW> sv_nx{}, pv_nx{};   // ... source and prediction row,
    unaligned_row<5> qp_nx{};                // ... the ten int16 quantiser parameters,
    short4 isc_nx[HOIST_ISCAN ? W / 4 : 1];  // ... inverse-scan row
    auto fetch_rows = [&](const svthip_tu_desc& d) {
#ifdef SVTHIP_TQ_EXP_NOMEM  // timing experiment (tools/build_variant.sh): no plane traffic, results meaningless
#pragma unroll
        for (int c = 0; c < ROWDW; c++) { sv_nx.v[c] = d.src_offset * 0x9e3779b1u + (uint32_t)(lane * 131 + c); pv_nx.v[c] = sv_nx.v[c] ^ 0x01030507u; }
#else
        sv_nx = *reinterpret_cast<const unaligned_row<ROWDW>*>(src + d.src_offset + (size_t)hi * d.src_stride);
        pv_nx = *reinterpret_cast<const unaligned_row<ROWDW>*>(pred + d.pred_offset + (size_t)hi * d.pred_stride);
#endif
        qp_nx = *reinterpret_cast<const unaligned_row<5>*>(qparams + (size_t)d.qparam_index * 10);
        if constexpr (HOIST_ISCAN) {
            const int16_t* iscan = iscan_pool + d.iscan_offset + hi * WIN;
#pragma unroll
            for (int c = 0; c < W / 4; c++) isc_nx[c] = *reinterpret_cast<const short4*>(iscan + 4 * c);
        }
    };
    // (the prefetches are unconditional, from a clamped TU index: a load under a condition puts its result into the loop-carried registers
    //  through copies right behind the load, i.e. waits for it on the spot)
    // The next descriptor is loaded as two raw 16-byte halves into registers that are NOT loop-carried and is unpacked behind an empty asm
    // after the column pass: unpacked where it is loaded, the compiler copies its fields into the loop-carried registers right behind the
    // load (s_waitcnt vmcnt + v_mov), one exposed memory round trip per group.
    struct RawDesc { unaligned_row<4> a, b; };
    auto load_desc_raw = [&](uint32_t tu) {
        const unaligned_row<4>* p = reinterpret_cast<const unaligned_row<4>*>(desc + tu);
        RawDesc r;
        r.a = p[0];
        r.b = p[1];
        return r;
    };
    auto unpack_desc = [](const RawDesc& r) {
        svthip_tu_desc d;
        d.src_offset = r.a.v[0];
        d.pred_offset = r.a.v[1];
        d.recon_offset = r.a.v[2];
        d.coeff_offset = r.a.v[3];
        d.iscan_offset = r.b.v[0];
        d.src_stride = (uint16_t)r.b.v[1];
        d.pred_stride = (uint16_t)(r.b.v[1] >> 16);
        d.recon_stride = (uint16_t)r.b.v[2];
        d.qparam_index = (uint16_t)(r.b.v[2] >> 16);
        d.tx_type = (uint8_t)r.b.v[3];
        return d;
    };
    static_assert(sizeof(svthip_tu_desc) == 32, "svthip_tu_desc is read as two 16-byte halves");
    if constexpr (PIPE) {
        if (n_tu == 0) return;
        const uint32_t grp0 = blockIdx.x * 4 + wave;
        d_nx = unpack_desc(load_desc_raw(min(grp0 * G + hg, n_tu - 1)));
        fetch_rows(d_nx);
    }
#ifdef SVTHIP_TQ_STAMPS  // debug build (tools/tq_stamps_probe.py): phase time stamps of every group's lane 0 into coeff_out (as uint64 [group][8])
    uint64_t stamp[8];
#define SVTHIP_STAMP(k) stamp[k] = __builtin_readcyclecounter()
#else
#define SVTHIP_STAMP(k)
#endif
    unaligned_row<ROWDW> o_dfr{};  // the previous group's reconstructed row, not stored yet
    PIX* o_ptr = nullptr;
    for (uint32_t grp = blockIdx.x * 4 + wave; grp < groups; grp += gstride) {
        SVTHIP_STAMP(0);
        svthip_tu_desc dh{};
        RawDesc rd_nx{};
        QParams QPh{};
        uint32_t ppk[ROWDW];
        short4 isc[HOIST_ISCAN ? W / 4 : 1];
        if constexpr (HOIST) {
            const int g = hg, i = hi;
            const uint32_t tu = grp * G + g;
            if constexpr (!PIPE) {
                if (tu < n_tu) {
                    d_nx = desc[tu];
                    fetch_rows(d_nx);
                }
            }
            // this group's operands were requested one group ago; the next group's descriptor goes out now
            dh = d_nx;
            const unaligned_row<ROWDW> sv = sv_nx, pv = pv_nx;
            const unaligned_row<5> qpr = qp_nx;
#pragma unroll
            for (int c = 0; c < (HOIST_ISCAN ? W / 4 : 1); c++) isc[c] = isc_nx[c];
            if constexpr (PIPE) {
                rd_nx = load_desc_raw(min((grp + gstride) * G + g, n_tu - 1));
#ifndef SVTHIP_TQ_EXP_NOMEM
                if (o_ptr) *reinterpret_cast<unaligned_row<ROWDW>*>(o_ptr) = o_dfr;
#endif
                o_ptr = nullptr;
            }
            if (tu < n_tu) {
#pragma unroll
                for (int k = 0; k < 2; k++) {  // {zbin, round, quant, quant_shift, dequant} x {DC, AC}, as load_qparams
                    const auto half = [&](int j) { return (int32_t)(int16_t)(qpr.v[j >> 1] >> (16 * (j & 1))); };
                    QPh.zb[k] = rpot(half(k), LOG_SCALE);
                    QPh.rnd[k] = rpot(half(2 + k), LOG_SCALE);
                    QPh.quant[k] = half(4 + k);
                    QPh.shift[k] = half(6 + k);
                    QPh.deq[k] = half(8 + k);
                }
                // ---- A0: residual of image row i into the tile (row H - 1 - i under the up-down flip of FLIPADST columns) ----
                const int kc = kVtx[dh.tx_type & 15];
                int32_t* row = tile + g * (H * P) + (kc == 2 ? H - 1 - i : i) * P;
#pragma unroll
                for (int c = 0; c < W; c++) {
                    const int32_t sc = (int32_t)((sv.v[c / PER] >> (PBITS * (c % PER))) & ((1u << PBITS) - 1u));
                    const int32_t pc = (int32_t)((pv.v[c / PER] >> (PBITS * (c % PER))) & ((1u << PBITS) - 1u));
                    row[c] = shift_val<SH0>(sc - pc);
                }
#pragma unroll
                for (int c = 0; c < ROWDW; c++) ppk[c] = pv.v[c];
            }
            wave_sync();
        }
        SVTHIP_STAMP(1);
        // ---- A: residual + forward column pass ----
#pragma unroll 1
        for (int round = 0; round < T::ROUNDS_COL; round++) {
            const int t = round * 64 + lane, g = t / W, c = t % W;
            const uint32_t tu = grp * G + g;
            if (tu < n_tu) {
                svthip_tu_desc d;
                if constexpr (HOIST) d = dh;
                else d = desc[tu];
                const int kc = kVtx[d.tx_type & 15], kr = kHtx[d.tx_type & 15];
                const PIX* s = src + d.src_offset + c;
                const PIX* p = pred + d.pred_offset + c;
                const int ss = d.src_stride, ps = d.pred_stride;
                int32_t x[H], y[H];
                if constexpr (HOIST) {
                    const int32_t* cin = tile + g * (H * P) + c;
#pragma unroll
                    for (int r = 0; r < H; r++) x[r] = cin[r * P];
                } else {
#pragma unroll
                    for (int r = 0; r < H; r++) {
                        const int rr = (kc == 2 ? H - 1 - r : r);
                        x[r] = shift_val<SH0>((int32_t)s[rr * ss] - (int32_t)p[rr * ps]);
                    }
                }
                txfm1d<H, BITC>(kc, x, y);
                int32_t* col = tile + g * (H * P) + (kr == 2 ? W - 1 - c : c);
#pragma unroll
                for (int r = 0; r < H; r++) col[r * P] = shift_val<SH1>(y[r]);
            }
        }
        wave_sync();
        SVTHIP_STAMP(2);
        if constexpr (PIPE) {
            asm volatile("" : "+v"(rd_nx.a.v[0]), "+v"(rd_nx.a.v[1]), "+v"(rd_nx.a.v[2]), "+v"(rd_nx.a.v[3]), "+v"(rd_nx.b.v[0]), "+v"(rd_nx.b.v[1]),
                         "+v"(rd_nx.b.v[2]), "+v"(rd_nx.b.v[3]));
            d_nx = unpack_desc(rd_nx);
            fetch_rows(d_nx);  // in flight during the row, inverse and reconstruction passes of this group
        }
        SVTHIP_STAMP(3);
        // ---- B: forward row pass, quantiser, inverse row pass ----
#pragma unroll 1
        for (int round = 0; round < T::ROUNDS_ROW; round++) {
            const int t = round * 64 + lane, g = t / H, r = t % H;
            const uint32_t tu = grp * G + g;
            const bool active = tu < n_tu;
            int64_t energy = 0, dist_res = 0, dist_pred = 0;  // sums of squares: non-negative, below 2^63
            int last = 0;
            if (active) {
                svthip_tu_desc d;
                if constexpr (HOIST) d = dh;
                else d = desc[tu];
                const int kr = kHtx[d.tx_type & 15];
                int32_t* row = tile + g * (H * P) + r * P;
                int32_t x[W], y[W];
#pragma unroll
                for (int c = 0; c < W; c++) x[c] = row[c];
                txfm1d<W, BITR>(kr, x, y);
#pragma unroll
                for (int c = 0; c < W; c++) {
                    y[c] = shift_val<SH2>(y[c]);
                    if constexpr (T::RECT2) y[c] = mulrs<12>(y[c], 5793);
                }
                if constexpr (W > 32 || H > 32) {
                    int64_t e4[4] = {0, 0, 0, 0};  // four independent chains: a single one would serialise on the mad latency
#pragma unroll
                    for (int c = 0; c < W; c++) {
                        if (c >= WIN) e4[c & 3] = mad64(y[c], y[c], e4[c & 3]);
                        else e4[c & 3] = mad64(r >= HIN ? y[c] : 0, y[c], e4[c & 3]);  // select, not a branch around the asm
                    }
                    energy = (e4[0] + e4[1]) + (e4[2] + e4[3]);
                }
                if (r < HIN) {
                    QParams QP;
                    if constexpr (HOIST) QP = QPh;
                    else QP = load_qparams(qparams + (size_t)d.qparam_index * 10, LOG_SCALE);
                    const int16_t* iscan = iscan_pool + d.iscan_offset + r * WIN;
                    const uint32_t base = d.coeff_offset + r * WIN;
                    int32_t dq[W];
#pragma unroll
                    for (int c = 0; c < WIN; c += 4) {
                        short4 is4;
                        if constexpr (HOIST_ISCAN) is4 = isc[c / 4];
                        else is4 = *reinterpret_cast<const short4*>(iscan + c);
                        const int isv[4] = {is4.x, is4.y, is4.z, is4.w};
                        int32_t qv[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            quant_one(y[c + k], (r | (c + k)) != 0, QP, LOG_SCALE, HIGHBD, qv[k], dq[c + k]);
                            if (qv[k] != 0) last = max(last, isv[k] + 1);
                            // coefficients and their reconstructions are far below 2^30 here (transform of 8/10-bit
                            // residuals), so the difference is exact in 32 bits and each square is one v_mad_i64_i32
                            if constexpr (!DIST) {
                            } else if constexpr (H > 32) {
                                // measured: with 64 rows per TU the plain C++ form is faster than the explicit mads
                                // (0.245 vs 0.36 ms per 16384 64x64 TUs), for every other height it is the other way round
                                const int64_t d64 = (int64_t)y[c + k] - dq[c + k];
                                dist_res += d64 * d64;
                                dist_pred += (int64_t)y[c + k] * y[c + k];
                            } else {
                                const int32_t dd = y[c + k] - dq[c + k];
                                dist_res = mad64(dd, dd, dist_res);
                                dist_pred = mad64(y[c + k], y[c + k], dist_pred);
                            }
                        }
                        if constexpr (QSTAGE) *reinterpret_cast<int4*>(qst + lane * QP_ + c) = make_int4(qv[0], qv[1], qv[2], qv[3]);
                        else *reinterpret_cast<int4*>(qcoeff_out + base + c) = make_int4(qv[0], qv[1], qv[2], qv[3]);
#ifndef SVTHIP_TQ_STAMPS
                        if (coeff_out) *reinterpret_cast<int4*>(coeff_out + base + c) = make_int4(y[c], y[c + 1], y[c + 2], y[c + 3]);
#endif
                        if (dqcoeff_out)
                            *reinterpret_cast<int4*>(dqcoeff_out + base + c) = make_int4(dq[c], dq[c + 1], dq[c + 2], dq[c + 3]);
                    }
                    // inverse row pass on the dequantised row (inv_txfm2d_add_c, EbTransforms.c:7648-7668)
                    int32_t xi[W], yi[W];
#pragma unroll
                    for (int c = 0; c < WIN; c++) {
                        int32_t v = dq[c];
                        if constexpr (T::RECT2) v = mulrs<12>(v, 2896);
                        xi[c] = lim.in(v);
                    }
#pragma unroll
                    for (int c = WIN; c < W; c++) xi[c] = 0;
                    itxfm1d<W, WIN>(kr, xi, yi, lim.in);
#pragma unroll
                    for (int c = 0; c < W; c++) {
                        if constexpr (ISH0 > 0) row[c] = rs<(ISH0 > 0 ? ISH0 : 1)>((int64_t)yi[c]);
                        else row[c] = yi[c];
                    }
                }
            }
            // per-TU reductions across the H lanes of the TU (inactive lanes contribute zeros)
            last = group_max_i32<H>(last);
            if constexpr (DIST) {
                dist_res = (int64_t)group_sum_u64<H>((uint64_t)dist_res);
                dist_pred = (int64_t)group_sum_u64<H>((uint64_t)dist_pred);
            }
            if constexpr (W > 32 || H > 32) energy = (int64_t)group_sum_u64<H>((uint64_t)energy);
            if constexpr (QSTAGE) {
                if (r == 0) qst[64 * QP_ + g] = (int32_t)(active ? dh.coeff_offset : 0xffffffffu);  // offsets are multiples of 4: all-ones marks a missing TU
            }
            if (active && r == 0) {
                eob_out[tu] = (uint16_t)last;
                if (energy_out) energy_out[tu] = (uint64_t)energy;
                if constexpr (DIST) {
                    dist_out[2 * (size_t)tu] = (uint64_t)dist_res;
                    dist_out[2 * (size_t)tu + 1] = (uint64_t)dist_pred;
                }
            }
        }
        wave_sync();
        if constexpr (QSTAGE) {
            // quad q = k * 64 + lane of the group's 64 x W coefficients: row R = q / (W / 4) of the image, TU R / H, row R % H of that TU
#pragma unroll
            for (int k = 0; k < W / 4; k++) {
                const int q = k * 64 + lane, R = q / (W / 4), cq = q % (W / 4);
                const int4 v = *reinterpret_cast<const int4*>(qst + R * QP_ + 4 * cq);
                const uint32_t off = (uint32_t)qst[64 * QP_ + R / H];
#ifdef SVTHIP_TQ_EXP_NOMEM
                if (off == 0xfffffff0u)
#else
                if (off != 0xffffffffu)
#endif
                    *reinterpret_cast<int4*>(qcoeff_out + off + (R % H) * W + 4 * cq) = v;
            }
        }
        SVTHIP_STAMP(4);
        // ---- C: inverse column pass + reconstruction ----
#pragma unroll 1
        for (int round = 0; round < T::ROUNDS_COL; round++) {
            const int t = round * 64 + lane, g = t / W, c = t % W;
            const uint32_t tu = grp * G + g;
            if (tu < n_tu) {
                svthip_tu_desc d;
                if constexpr (HOIST) d = dh;
                else d = desc[tu];
                const int kc = kVtx[d.tx_type & 15], kr = kHtx[d.tx_type & 15];
                const int32_t* col = tile + g * (H * P) + (kr == 2 ? W - 1 - c : c);
                int32_t x[H], y[H];
#pragma unroll
                for (int r = 0; r < HIN; r++) x[r] = lim.col(col[r * P]);
#pragma unroll
                for (int r = HIN; r < H; r++) x[r] = 0;
                itxfm1d<H, HIN>(kc, x, y, lim.col);
                const PIX* p = pred + d.pred_offset + c;
                PIX* out = recon + d.recon_offset + c;
                const int ps = d.pred_stride, rs_ = d.recon_stride;
                if constexpr (HOIST) {
                    int32_t* cout_ = tile + g * (H * P) + c;  // image column c, image rows (every lane has read its input column by now)
#pragma unroll
                    for (int r = 0; r < H; r++) cout_[flip_row<H>(r, kc) * P] = lim.residual(rs<4>((int64_t)y[r]));
                } else {
#pragma unroll
                    for (int r = 0; r < H; r++) {
                        const int32_t t = lim.residual(rs<4>((int64_t)y[r]));
                        const int rr = flip_row<H>(r, kc);
                        const int32_t v = (int32_t)p[rr * ps] + t;
                        out[rr * rs_] = (PIX)min(max(v, 0), lim.pix_max);
                    }
                }
            }
        }
        wave_sync();
        SVTHIP_STAMP(5);
        // ---- D (square sizes): reconstruction by rows ----
        if constexpr (HOIST) {
            const int g = lane / W, i = lane % W;
            const uint32_t tu = grp * G + g;
            if (tu < n_tu) {
                const int32_t* row = tile + g * (H * P) + i * P;
                unaligned_row<ROWDW> o;
#pragma unroll
                for (int c = 0; c < ROWDW; c++) {
                    uint32_t pk = 0;
#pragma unroll
                    for (int k = 0; k < PER; k++) {
                        const int32_t pc = (int32_t)((ppk[c] >> (PBITS * k)) & ((1u << PBITS) - 1u));
                        const int32_t v = min(max(pc + row[c * PER + k], 0), lim.pix_max);
                        pk |= (uint32_t)v << (PBITS * k);
                    }
                    o.v[c] = pk;
                }
                PIX* optr = recon + dh.recon_offset + (size_t)i * dh.recon_stride;
                if constexpr (PIPE) {  // stored at the top of the wave's next group: the loop-carried prefetch makes the end of a group wait for
                    o_dfr = o;         // everything in flight, and a store issued here would be waited for at once
                    o_ptr = optr;
                } else {
                    *reinterpret_cast<unaligned_row<ROWDW>*>(optr) = o;
                }
            }
            wave_sync();
        }
#ifdef SVTHIP_TQ_STAMPS
        SVTHIP_STAMP(6);
        if (lane == 0 && coeff_out) {
            stamp[7] = ((uint64_t)blockIdx.x << 8) | (uint64_t)wave;
#pragma unroll
            for (int k = 0; k < 8; k++) reinterpret_cast<uint64_t*>(coeff_out)[(size_t)grp * 8 + k] = stamp[k];
        }
#endif
    }
    if constexpr (PIPE) {
        if (o_ptr) *reinterpret_cast<unaligned_row<ROWDW>*>(o_ptr) = o_dfr;
    }
}

template <typename T, typename PIX>
hipError_t launch_one(const PIX* src, const PIX* pred, PIX* recon, const svthip_tu_desc* desc, uint32_t n_tu,
                      const int16_t* qparams, const int16_t* iscan, int32_t* coeff, int32_t* qcoeff, int32_t* dqcoeff, uint16_t* eob,
                      uint64_t* energy, uint64_t* dist, uint32_t max_wg, hipStream_t s)
{
    constexpr int WL = T::WL, HL = T::HL;
    constexpr size_t lds = T::lds_bytes(true);
    uint32_t blocks = T::blocks(n_tu);
    if constexpr (T::PIPE) {  // waves walk several groups, prefetching
        // as many workgroups as the chip holds at once (all of one kernel variant's launches run on one GPU model)
        static const uint32_t resident = [] {
            int dev = 0, cus = 256, per_cu = 0;
            if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&encode_tu_kernel<WL, HL, PIX, false>), 256, lds) !=
                    hipSuccess || per_cu < 1)
                per_cu = 2;
            return (uint32_t)(cus * per_cu);
        }();
        if (blocks > 2 * resident) blocks = resident;  // up to two rounds of workgroups there is nothing to walk
    }
    if (max_wg && blocks > max_wg) blocks = max_wg;  // SVTHIP_OPT_TQ_MAX_WORKGROUPS (every kernel form walks its groups grid-stride)
    const auto kernel = dist ? &encode_tu_kernel<WL, HL, PIX, true> : &encode_tu_kernel<WL, HL, PIX, false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, s, src, pred, recon, desc, n_tu, qparams, iscan, coeff, qcoeff, dqcoeff, eob, energy, dist);
    return hipGetLastError();
}

template <typename PIX>
hipError_t launch_sized(const PIX* src, const PIX* pred, PIX* recon, const svthip_tu_desc* desc, uint32_t n_tu, int w, int h,
                        const int16_t* qparams, const int16_t* iscan, int32_t* coeff, int32_t* qcoeff, int32_t* dqcoeff, uint16_t* eob,
                        uint64_t* energy, uint64_t* dist, uint32_t max_wg, hipStream_t s)
{
    return tx_size_dispatch(w, h, hipErrorInvalidValue, [&](auto tile) {
        return launch_one<decltype(tile), PIX>(src, pred, recon, desc, n_tu, qparams, iscan, coeff, qcoeff, dqcoeff, eob, energy, dist, max_wg, s);
    });
}

}  // namespace

hipError_t launch_encode_tu(const void* src, const void* pred, void* recon, int planes_16bit, const svthip_tu_desc* desc, uint32_t n_tu,
                            int w, int h, const int16_t* qparams, const int16_t* iscan, int32_t* coeff, int32_t* qcoeff,
                            int32_t* dqcoeff, uint16_t* eob, uint64_t* energy, uint64_t* dist, uint32_t max_workgroups, hipStream_t s)
{
    if (planes_16bit)
        return launch_sized<uint16_t>(static_cast<const uint16_t*>(src), static_cast<const uint16_t*>(pred), static_cast<uint16_t*>(recon),
                                      desc, n_tu, w, h, qparams, iscan, coeff, qcoeff, dqcoeff, eob, energy, dist, max_workgroups, s);
    return launch_sized<uint8_t>(static_cast<const uint8_t*>(src), static_cast<const uint8_t*>(pred), static_cast<uint8_t*>(recon), desc,
                                 n_tu, w, h, qparams, iscan, coeff, qcoeff, dqcoeff, eob, energy, dist, max_workgroups, s);
}

hipError_t encode_tu_raise_dynamic_lds()
{
    const void* list[4 * 19];
    size_t n = 0;
#define ADD(WL, HL)                                                                                                                             \
    if (TxTile<WL, HL>::lds_bytes(true) > kDefaultDynamicLdsLimit)                                                                              \
        for (const void* k : {(const void*)&encode_tu_kernel<WL, HL, uint8_t, false>, (const void*)&encode_tu_kernel<WL, HL, uint8_t, true>,    \
                              (const void*)&encode_tu_kernel<WL, HL, uint16_t, false>, (const void*)&encode_tu_kernel<WL, HL, uint16_t, true>}) \
            list[n++] = k;
    SVTHIP_TX_SIZES(ADD)
#undef ADD
    return raise_dynamic_lds(list, n);
}

}  // namespace svthip
