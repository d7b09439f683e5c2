// svt-av1-1_amd/csrc/ip_intra.hip
//
// AV1 intra prediction of transform blocks: a batch of blocks of one TxSize, each what one call of build_intra_predictors /
// build_intra_predictors_high writes (Source/Lib/Codec/EbIntraPrediction.c:8823-9080 / :9082-9317) as the reference is configured:
// no edge filter, no upsampling (DIS_EDGE_FIL), no filter-intra, no palette.
//
//   mapping    intra_pred_kernel<HBD, TXW, TXH>: a lane writes four consecutive samples of a row (a quad).  A block of TXW x TXH is
//              TXW / 4 * TXH quads and is worked by G = min(64, quads) lanes, so a wave holds 64 / G blocks (sixteen 4x4, four 8x8, one
//              of 16x16 and above) and a block of more than 64 quads is walked in passes of 16 (TXW = 64) .. 4 (TXW = 16) rows.  A block
//              never spans waves, so nothing but wave-local ordering is needed after the table is staged.
//   edges      above_row[-1 .. TXW + TXH) and left_col[-1 .. TXW + TXH) are built in LDS as 16-bit values, always both and always whole,
//              the way generate_intra_reference_samples (:8531) builds them for mode decision: available samples, then the last one
//              repeated; a missing side takes the other side's first sample or base -+ 1; the corner by the reference's rule.  The
//              EncDec path builds only what the mode reads and fills the block with one value when the mode's only edge is missing; with
//              a constant edge every predictor of that mode gives that value, so one build serves both paths.
//   predict    DC (the four dc_pred arms, the sum by a butterfly over the block's lanes), V, H, SMOOTH / _V / _H, PAETH, and the
//              directional zones 1 / 2 / 3 of dr_predictor (:7984) with the step from Dr_Intra_Derivative.  With one block per wave the
//              descriptor sits in scalar registers and the mode switch is a scalar branch; with several blocks per wave the lanes of
//              different modes diverge.
//   stores     one dword (8 bits) or one qword (16 bits) per quad when the address allows, else per sample.
//   SAD        8-bit, optional: v_sad_u8 of the packed quad against the source, summed over the block's lanes.
//
// A descriptor that breaks one of the reference's asserts (mode, angle delta, a count above the block side, top-right without a whole
// top, bottom-left without a whole left) is refused: nothing is written for it and the context's counter is incremented once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/svtav1_hip.h"
#include "ip_launch.h"

static_assert(sizeof(svthip_intra_desc) == 32, "svthip_intra_desc is 32 bytes (include/svtav1_hip.h)");

namespace svthip {

namespace {

#include "av1_intra_tables.inc"

struct IntraArgs {
    const void* edge;
    void* dst;
    const svthip_intra_desc* desc;
    uint32_t n;
    const uint8_t* src;
    uint32_t* sad;
    uint32_t* refused;
    int bd;
};

// mode_to_angle_map of the directional modes V_PRED .. D67_PRED (PredictionMode 1 .. 8)
__device__ const uint8_t kModeAngle[9] = {0, 90, 180, 45, 135, 113, 157, 203, 67};

enum Kind { K_DC, K_V, K_H, K_SMOOTH, K_SMOOTH_V, K_SMOOTH_H, K_PAETH, K_Z1, K_Z2, K_Z3 };

// sum over the G lanes of a block (G a power of two, the lanes aligned to it)
template <int G>
__device__ __forceinline__ uint32_t group_sum(uint32_t v)
{
#pragma unroll
    for (int m = G >> 1; m > 0; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

template <bool HBD, int TXW, int TXH>
__global__ void __launch_bounds__(256) intra_pred_kernel(IntraArgs A)
{
    using T = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    constexpr int N = TXW + TXH, QW = TXW / 4, QUADS = QW * TXH, G = QUADS < 64 ? QUADS : 64, J = 64 / G;
    constexpr int ES = N + 4;  // [3] = sample -1, [4 + i] = sample i: sample 0 is 8-byte aligned
    __shared__ uint16_t edges[4 * J][2][ES];
    __shared__ uint8_t smw[128];
    if (threadIdx.x < 128) smw[threadIdx.x] = kSmWeights[threadIdx.x];
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int g = lane / G, l = lane % G;
    const uint32_t job = (blockIdx.x * 4u + (uint32_t)wave) * J + (uint32_t)g;
    if (job >= A.n) return;
    const uint4* dp = reinterpret_cast<const uint4*>(A.desc + job);
    const uint4 d0 = dp[0], d1 = dp[1];
    const uint32_t above_offset = d0.x, left_offset = d0.y, left_stride = d0.z, dst_offset = d0.w, dst_stride = d1.x;
    const int n_top = d1.y & 255, n_tr = (d1.y >> 8) & 255, n_left = (d1.y >> 16) & 255, n_bl = d1.y >> 24;
    const int mode = d1.z & 255, delta = (int8_t)((d1.z >> 8) & 255);
    const uint32_t src_stride = d1.z >> 16, src_offset = d1.w;

    if (mode > 12 || delta < -3 || delta > 3 || n_top > TXW || n_tr > TXW || n_left > TXH || n_bl > TXH || (n_tr > 0 && n_top != TXW) ||
        (n_bl > 0 && n_left != TXH)) {
        if (l == 0) atomicAdd(A.refused, 1u);
        return;
    }

    // ---- the two edges ----
    uint16_t* ab = &edges[wave * J + g][0][4];
    uint16_t* lf = &edges[wave * J + g][1][4];
    const T* aref = static_cast<const T*>(A.edge) + above_offset;
    const T* lref = static_cast<const T*>(A.edge) + left_offset;
    const int base = HBD ? 128 << (A.bd - 8) : 128;
    {
        const int nt = n_top + n_tr, nl = n_left + n_bl;
        const int fill_a = n_left > 0 ? (int)lref[0] : base - 1, fill_l = n_top > 0 ? (int)aref[0] : base + 1;
        for (int i = l; i < N; i += G) {
            ab[i] = (uint16_t)(n_top > 0 ? (int)aref[min(i, nt - 1)] : fill_a);
            lf[i] = (uint16_t)(n_left > 0 ? (int)lref[(size_t)min(i, nl - 1) * left_stride] : fill_l);
        }
        if (l == 0) {
            const int corner = n_top > 0 ? (n_left > 0 ? (int)aref[-1] : fill_l) : (n_left > 0 ? fill_a : base);
            ab[-1] = lf[-1] = (uint16_t)corner;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- what to run: mode_to_angle_map + 3 delta chooses the zone; exactly 90 / 180 are V / H ----
    int kind, dx = 0, dy = 0;
    if (mode >= 1 && mode <= 8) {
        const int p = kModeAngle[mode] + 3 * delta;
        if (p == 90) kind = K_V;
        else if (p == 180) kind = K_H;
        else if (p < 90) { kind = K_Z1; dx = kDrIntraDerivative[p]; }
        else if (p < 180) { kind = K_Z2; dx = kDrIntraDerivative[180 - p]; dy = kDrIntraDerivative[p - 90]; }
        else { kind = K_Z3; dy = kDrIntraDerivative[270 - p]; }
    } else {
        kind = mode == 0 ? K_DC : mode == 9 ? K_SMOOTH : mode == 10 ? K_SMOOTH_V : mode == 11 ? K_SMOOTH_H : K_PAETH;
    }

    int dc = base;
    if (kind == K_DC && (n_top > 0 || n_left > 0)) {
        uint32_t s = 0;
        if (n_top > 0)
            for (int i = l; i < TXW; i += G) s += ab[i];
        if (n_left > 0)
            for (int i = l; i < TXH; i += G) s += lf[i];
        s = group_sum<G>(s);
        if (n_top > 0 && n_left > 0) dc = (int)((s + (uint32_t)(N >> 1)) / (uint32_t)N);
        else if (n_top > 0) dc = (int)((s + (uint32_t)(TXW >> 1)) / (uint32_t)TXW);
        else dc = (int)((s + (uint32_t)(TXH >> 1)) / (uint32_t)TXH);
    }
    const int below = lf[TXH - 1], right = ab[TXW - 1], tl = ab[-1];

    T* dst = static_cast<T*>(A.dst) + dst_offset;
    const uint8_t* src = A.src + src_offset;
    uint32_t sad = 0;
#pragma unroll 1
    for (int q = l; q < QUADS; q += G) {
        const int r = q / QW, c0 = (q % QW) * 4;
        int v[4];
        switch (kind) {
        case K_DC:
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = dc;
            break;
        case K_V:
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = ab[c0 + k];
            break;
        case K_H:
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = lf[r];
            break;
        case K_SMOOTH: {
            const int wh = smw[TXH + r], lr = lf[r];
            const int rowpart = (256 - wh) * below + 256;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int ww = smw[TXW + c0 + k];
                v[k] = (wh * (int)ab[c0 + k] + rowpart + ww * lr + (256 - ww) * right) >> 9;
            }
            break;
        }
        case K_SMOOTH_V: {
            const int wh = smw[TXH + r];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = (wh * (int)ab[c0 + k] + (256 - wh) * below + 128) >> 8;
            break;
        }
        case K_SMOOTH_H: {
            const int lr = lf[r];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int ww = smw[TXW + c0 + k];
                v[k] = (ww * lr + (256 - ww) * right + 128) >> 8;
            }
            break;
        }
        case K_PAETH: {
            const int lr = lf[r];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int top = ab[c0 + k], b = top + lr - tl;
                const int pl = iabs(b - lr), pt = iabs(b - top), ptl = iabs(b - tl);
                v[k] = (pl <= pt && pl <= ptl) ? lr : (pt <= ptl ? top : tl);
            }
            break;
        }
        case K_Z1: {
            const int x = (r + 1) * dx, sh = (x & 63) >> 1, b0 = (x >> 6) + c0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int b = min(b0 + k, N - 1);
                const int two = (int)ab[b] * (32 - sh) + (int)ab[min(b + 1, N - 1)] * sh;
                v[k] = b0 + k < N - 1 ? (two + 16) >> 5 : (int)ab[N - 1];
            }
            break;
        }
        case K_Z3: {
            // no tail arm: the steepest legal angle (203 + 9 degrees) steps 40 / 64 of a sample per column, so the base stays at or
            // below TXW * 40 / 64 + TXH - 1 < N - 1 and base + 1 is inside the edge
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int y = (c0 + k + 1) * dy, sh = (y & 63) >> 1, b = (y >> 6) + r;
                v[k] = ((int)lf[b] * (32 - sh) + (int)lf[b + 1] * sh + 16) >> 5;
            }
            break;
        }
        default: {  // K_Z2
            const int x = -(r + 1) * dx, sh1 = (x & 63) >> 1, b0 = (x >> 6) + c0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int b1 = b0 + k;
                const int y = (r << 6) - (c0 + k + 1) * dy, b2 = max(y >> 6, -1), sh2 = (y & 63) >> 1;
                const bool up = b1 >= -1;
                const uint16_t* e = up ? ab : lf;
                const int b = up ? b1 : b2, sh = up ? sh1 : sh2;
                v[k] = ((int)e[b] * (32 - sh) + (int)e[b + 1] * sh + 16) >> 5;
            }
            break;
        }
        }
        T* p = dst + (size_t)r * dst_stride + c0;
        if (HBD) {
            if ((reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
                *reinterpret_cast<uint2*>(p) = uint2{(uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16)};
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) p[k] = (T)v[k];
            }
        } else {
            const uint32_t packed = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
            if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
                *reinterpret_cast<uint32_t*>(p) = packed;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) p[k] = (T)v[k];
            }
            if (A.sad) {
                const uint8_t* sp = src + (size_t)r * src_stride + c0;
                uint32_t s4;
                if ((reinterpret_cast<uintptr_t>(sp) & 3u) == 0) s4 = *reinterpret_cast<const uint32_t*>(sp);
                else s4 = (uint32_t)sp[0] | ((uint32_t)sp[1] << 8) | ((uint32_t)sp[2] << 16) | ((uint32_t)sp[3] << 24);
                sad = __builtin_amdgcn_sad_u8(packed, s4, sad);
            }
        }
    }
    if (!HBD && A.sad) {
        sad = group_sum<G>(sad);
        if (l == 0) A.sad[job] = sad;
    }
}

constexpr uint8_t kTxW[19] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64};
constexpr uint8_t kTxH[19] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16};

template <bool HBD, int S>
hipError_t launch_size(const IntraArgs& A, hipStream_t s)
{
    constexpr int W = kTxW[S], H = kTxH[S], QUADS = W / 4 * H, G = QUADS < 64 ? QUADS : 64, per_group = 4 * (64 / G);
    const uint64_t groups = ((uint64_t)A.n + per_group - 1) / per_group;
    if (groups > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((intra_pred_kernel<HBD, W, H>), dim3((uint32_t)groups), dim3(256), 0, s, A);
    return hipGetLastError();
}

template <bool HBD>
hipError_t launch_depth(const IntraArgs& A, int tx_size, hipStream_t s)
{
    switch (tx_size) {
#define SVTHIP_INTRA_CASE(S) case S: return launch_size<HBD, S>(A, s);
        SVTHIP_INTRA_CASE(0) SVTHIP_INTRA_CASE(1) SVTHIP_INTRA_CASE(2) SVTHIP_INTRA_CASE(3) SVTHIP_INTRA_CASE(4) SVTHIP_INTRA_CASE(5)
        SVTHIP_INTRA_CASE(6) SVTHIP_INTRA_CASE(7) SVTHIP_INTRA_CASE(8) SVTHIP_INTRA_CASE(9) SVTHIP_INTRA_CASE(10) SVTHIP_INTRA_CASE(11)
        SVTHIP_INTRA_CASE(12) SVTHIP_INTRA_CASE(13) SVTHIP_INTRA_CASE(14) SVTHIP_INTRA_CASE(15) SVTHIP_INTRA_CASE(16) SVTHIP_INTRA_CASE(17)
        SVTHIP_INTRA_CASE(18)
#undef SVTHIP_INTRA_CASE
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

bool intra_tx_size_valid(uint32_t tx_size) { return tx_size < 19; }

hipError_t launch_intra_pred(const void* edge, void* dst, const svthip_intra_desc* desc, uint32_t n_blocks, int tx_size, int bd, const uint8_t* src,
                             uint32_t* sad, uint32_t* refused, hipStream_t s)
{
    IntraArgs A{edge, dst, desc, n_blocks, src, sad, refused, bd};
    return bd > 8 ? launch_depth<true>(A, tx_size, s) : launch_depth<false>(A, tx_size, s);
}

}  // namespace svthip
