// svt-av1-1_amd/csrc/tq_fwd_txfm.hip
//
// Batched forward 2-D transforms for AV1 transform units, gfx950.  Replaces Av1TransformTwoD_{4x4..64x64}_c and
// av1_fwd_txfm2d_{WxH}_c (Source/Lib/Codec/EbTransforms.c:3928-4400) = Av1TranformTwoDCore_c (:3701-3780) configured by
// Av1TransformConfig (:3847-3867), with the 1-D networks av1_fdct{4,8,16,32,64}_new (:1314-2762),
// av1_fadst{4,8,16}_new (:2764-3183) and av1_fidentity{4,8,16,32}_c.
//
// Mapping.  One launch handles TUs of one size W x H.  A wave owns G = 64 / min(W, H) TUs at a time (TxTile, tq_tile.h), so the pass whose
// lanes run along the shorter dimension fills the wave exactly and the other pass takes max / min rounds of 64 lanes:
//   column pass: lane = (tu, column); the lane loads its H residuals (2-byte loads, a row of a TU is contiguous across lanes),
//                runs the whole 1-D network in registers (every index is a compile-time constant, so the arrays below are
//                VGPRs) and writes the rounded column into the wave's LDS tile (pitch W + 1 words: conflict-free both ways);
//   row pass:    lane = (tu, row); reads its row from LDS, runs the row network in registers, applies shift[2] and the
//                2:1-rectangle sqrt(2) scaling, and stores W contiguous int32.
// No cross-lane traffic inside a network; the only exchange is the LDS transpose between the passes.
//
// Arithmetic.  half_btf (:1292-1299) = round_shift(w0*in0 + w1*in1, cos_bit) with an int64 sum; here the two products are
// formed by v_mad_i64_i32 (full 64-bit products).  They equal the reference's int32 products on every input for which the
// reference is defined (its stage ranges keep w*in inside int32; signed overflow there is undefined behaviour in C), so the
// results are bit-identical for residuals of 8- and 10-bit video.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svtav1_hip.h"
#include "tq_launch.h"
#include "tq_tile.h"

namespace svthip {

namespace {

#include "tq_txfm_common.h"

#include "tq_fwd_networks.h"

template <int WL, int HL>
__global__ void __launch_bounds__(256) fwd_txfm2d_kernel(const int16_t* __restrict__ residual, const svthip_txfm_desc* __restrict__ desc,
                                                         uint32_t n_tu, int32_t* __restrict__ coeff)
{
    using T = TxTile<WL, HL>;
    constexpr int W = T::W, H = T::H, G = T::G, P = T::P;
    constexpr int SH0 = kShift[T::WI][T::HI][0], SH1 = kShift[T::WI][T::HI][1], SH2 = kShift[T::WI][T::HI][2];
    constexpr int BITC = kCosCol[T::WI][T::HI], BITR = kCosRow[T::WI][T::HI];
    // rows of >= 16 coefficients leave through LDS with coalesced stores (measured: +10..15 % at 16x16 .. 64x64, -10 % at 4x4 / 8x8)
    constexpr bool STAGED_OUT = W >= 16;
    extern __shared__ int32_t lds_all[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t* tile = lds_all + wave * T::tile_words;
    const uint32_t groups = T::groups(n_tu);
    for (uint32_t grp = blockIdx.x * 4 + wave; grp < groups; grp += gridDim.x * 4) {
        // ---- column pass ----
#pragma unroll 1
        for (int round = 0; round < T::ROUNDS_COL; round++) {
            const int t = round * 64 + lane, g = t / W, c = t % W;
            const uint32_t tu = grp * G + g;
            if (tu < n_tu) {
                const svthip_txfm_desc d = desc[tu];
                const int kc = kVtx[d.tx_type & 15], kr = kHtx[d.tx_type & 15];
                const int16_t* in = residual + d.in_offset + c;
                const int stride = d.in_stride;
                int32_t x[H], y[H];
#pragma unroll
                for (int r = 0; r < H; r++) x[r] = shift_val<SH0>((int32_t)in[(kc == 2 ? H - 1 - r : r) * stride]);
                txfm1d<H, BITC>(kc, x, y);
                int32_t* col = tile + g * (H * P) + (kr == 2 ? W - 1 - c : c);
#pragma unroll
                for (int r = 0; r < H; r++) col[r * P] = shift_val<SH1>(y[r]);
            }
        }
        wave_sync();
        // ---- row pass ----
#pragma unroll 1
        for (int round = 0; round < T::ROUNDS_ROW; round++) {
            const int t = round * 64 + lane, g = t / H, r = t % H;
            const uint32_t tu = grp * G + g;
            if (tu < n_tu) {
                const svthip_txfm_desc d = desc[tu];
                const int kr = kHtx[d.tx_type & 15];
                const int32_t* row = tile + g * (H * P) + r * P;
                int32_t x[W], y[W];
#pragma unroll
                for (int c = 0; c < W; c++) x[c] = row[c];
                txfm1d<W, BITR>(kr, x, y);
                if constexpr (STAGED_OUT) {
                    // the finished row goes back to the same LDS row (only this lane touches it between the two barriers) ...
                    int32_t* orow = tile + g * (H * P) + r * P;
#pragma unroll
                    for (int c = 0; c < W; c++) {
                        int32_t v = shift_val<SH2>(y[c]);
                        if constexpr (T::RECT2) v = mulrs<12>(v, 5793);
                        orow[c] = v;
                    }
                } else {
                    int32_t* out = coeff + d.out_offset + r * W;
#pragma unroll
                    for (int c = 0; c < W; c += 4) {
                        int32_t v[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            v[k] = shift_val<SH2>(y[c + k]);
                            if constexpr (T::RECT2) v[k] = mulrs<12>(v[k], 5793);
                        }
                        *reinterpret_cast<int4*>(out + c) = make_int4(v[0], v[1], v[2], v[3]);
                    }
                }
            }
        }
        if constexpr (STAGED_OUT) {
            wave_sync();
            // ... and the group's coefficients leave with coalesced 16-byte stores (a TU is one contiguous run of W * H int32)
            constexpr int NQ = W * H / 4;
#pragma unroll 4
            for (int i = lane; i < G * NQ; i += 64) {
                const int g = i / NQ, q = i - g * NQ;
                const uint32_t tu = grp * G + g;
                if (tu < n_tu) {
                    const int r = (4 * q) / W, c = (4 * q) % W;
                    const int32_t* src = tile + g * (H * P) + r * P + c;
                    *reinterpret_cast<int4*>(coeff + desc[tu].out_offset + 4 * q) = make_int4(src[0], src[1], src[2], src[3]);
                }
            }
        }
        wave_sync();
    }
}

}  // namespace

bool fwd_txfm2d_size_valid(int w, int h) { return tx_size_dispatch(w, h, false, [](auto) { return true; }); }

// (size, tx_type) combinations for which the reference has a 1-D network (ADST up to 16 points, identity up to 32)
bool fwd_txfm2d_type_valid(int w, int h, int tx_type)
{
    if (tx_type < 0 || tx_type > 15) return false;
    const int kc = kVtx[tx_type], kr = kHtx[tx_type];
    if ((kc == 1 || kc == 2) && h > 16) return false;
    if ((kr == 1 || kr == 2) && w > 16) return false;
    if (kc == 3 && h > 32) return false;
    if (kr == 3 && w > 32) return false;
    return true;
}

hipError_t launch_fwd_txfm2d(const int16_t* residual, const svthip_txfm_desc* desc, uint32_t n_tu, int w, int h, int32_t* coeff,
                             hipStream_t s)
{
    return tx_size_dispatch(w, h, hipErrorInvalidValue, [&](auto tile) {
        using T = decltype(tile);
        hipLaunchKernelGGL((fwd_txfm2d_kernel<T::WL, T::HL>), dim3(T::blocks(n_tu)), dim3(256), T::lds_bytes(), s, residual, desc, n_tu, coeff);
        return hipGetLastError();
    });
}

hipError_t fwd_txfm_raise_dynamic_lds()
{
    const void* list[19];
    size_t n = 0;
#define ADD(WL, HL) \
    if (TxTile<WL, HL>::lds_bytes() > kDefaultDynamicLdsLimit) list[n++] = reinterpret_cast<const void*>(&fwd_txfm2d_kernel<WL, HL>);
    SVTHIP_TX_SIZES(ADD)
#undef ADD
    return raise_dynamic_lds(list, n);
}

}  // namespace svthip
