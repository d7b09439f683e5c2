// svt-av1-1_amd/csrc/lr_wiener.hip -- Wiener loop restoration on the device: per-unit statistics, the separable solve, the unit filter (as
// SSE trial and as frame filter) and the refinement walk as a state machine.  Restates Codec/EbRestorationPick.c:743-1104, :1257-1366,
// EbRestoration.c:198-237, :346-554, :1172-1246, :1343-1389 and convolve.c:64-222; the contract is in include/svtav1_hip.h.
// Not here: self-guided restoration, rest_finish_search, CDEF, 12 bits, superres, more than one tile.
#include "me_kernels.h"

namespace svthip {

namespace {

constexpr int kTapMid[3] = {3, -7, 15};   // WIENER_FILT_TAPn_MIDV
constexpr int kTapBits[3] = {4, 5, 6};    // WIENER_FILT_TAPn_BITS
__host__ __device__ constexpr int tap_min(int p) { return kTapMid[p] - (1 << kTapBits[p]) / 2; }
__host__ __device__ constexpr int tap_max(int p) { return kTapMid[p] - 1 + (1 << kTapBits[p]) / 2; }
constexpr int kFiltStep = 128;                     // WIENER_FILT_STEP
constexpr int64_t kTapScale = (int64_t)1 << 16;    // WIENER_TAP_SCALE_FACTOR
constexpr int kNumIters = 5;                       // NUM_WIENER_ITERS
// Lanes per workgroup of the tiled kernels.  tests/test_lr_kernels_host.py compiles the kernel bodies below for the host with one lane
// per workgroup (which then does all of its workgroup's work in order) to check them against the fixture without a GPU.
#ifndef SVTHIP_LR_THREADS
#define SVTHIP_LR_THREADS 256
#endif
constexpr int kThreads = SVTHIP_LR_THREADS;

// ---------------------------------------------------------------- geometry: the one place (host, binding through the ABI, kernels)
struct PlaneGeom {
    int w, h, unit, ss, nx, ny, base, win;
};
struct Limits {
    int h0, h1, v0, v1;
};

__host__ __device__ inline int units_in(int size, int unit)
{
    const int n = (size + (unit >> 1)) / unit;
    return n < 1 ? 1 : n;
}

__host__ __device__ inline PlaneGeom plane_geom(uint32_t width, uint32_t height, const uint32_t unit_size[3], int plane)
{
    PlaneGeom g{};
    int base = 0;
    for (int p = 0; p <= plane; p++) {
        g.ss = p > 0;
        g.w = (int)width >> g.ss, g.h = (int)height >> g.ss, g.unit = (int)unit_size[p];
        g.nx = units_in(g.w, g.unit), g.ny = units_in(g.h, g.unit);
        g.base = base;
        base += g.nx * g.ny;
    }
    g.win = plane ? 5 : 7;
    return g;
}

// Unit i of a row or column starts at i * unit; the last one takes what remains (less than 1.5 units, by the rounding of units_in).
// Vertically every unit but the first starts 8 >> ss rows early and every unit but the last ends that much early.
__host__ __device__ inline Limits unit_limits(const PlaneGeom& g, int i)
{
    const int ux = i % g.nx, uy = i / g.nx, off = 8 >> g.ss;
    Limits L;
    L.h0 = ux * g.unit;
    L.h1 = ux == g.nx - 1 ? g.w : (ux + 1) * g.unit;
    L.v0 = uy == 0 ? 0 : uy * g.unit - off;
    L.v1 = uy == g.ny - 1 ? g.h : (uy + 1) * g.unit - off;
    return L;
}

__host__ __device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// ---------------------------------------------------------------- statistics
// One workgroup sums one 32x32 tile of a unit.  With Z = (the win^2 window samples, the source sample, 1) per pixel, every sum the
// statistics need is a sum of products Z_k * Z_l, k <= l: the Gram matrix of the window (H), window x source (M), the plain sums (for
// avg, which is then needed only in the integer epilogue: sum (d - a)(d' - a) = sum d d' - a sum d - a sum d' + N a^2), source^2 (with M
// and H at the centre: the SSE of the unrestored unit).  A lane owns up to 6 of the (win^2 + 2)(win^2 + 3) / 2 - 1 products and keeps each
// tile sum in 32 bits: a product of raw samples is below 2^20 at 10 bits (2^16 at 8), so 1024 pixels stay below 2^30 (2^26); a 64x64
// tile would not at 10 bits.  The tile sums are added to the unit's in 64 bits with integer atomics, whose order does not matter.
constexpr int kStatTile = 32;
constexpr int kStatPitch = 40;                        // LDS row pitch in samples: window rows 0..6 start on distinct bank groups
constexpr int kStatRowsD = kStatTile + 6;             // window tile with its halo
constexpr int kStatItemsPerLane = (1325 + kThreads - 1) / kThreads;   // 6 with 256 lanes
constexpr int kRawStride = 1328;                      // 64-bit sums per unit: 51 * 52 / 2 - 1 = 1325, padded

__host__ __device__ inline int tri_index(int k, int l, int nz) { return k * nz - k * (k - 1) / 2 + (l - k); }  // k <= l

template <typename T>
__global__ __launch_bounds__(kThreads) void lr_stats_kernel(const T* __restrict__ dgd, uint32_t dgd_stride, const T* __restrict__ src, uint32_t src_stride,
                                                        PlaneGeom g, unsigned long long* __restrict__ raw)
{
    __shared__ uint16_t buf[(kStatRowsD + 2 * kStatTile) * kStatPitch];
    const int u = blockIdx.z, tid = threadIdx.x;
    const Limits L = unit_limits(g, u);
    const int tx0 = L.h0 + (int)blockIdx.x * kStatTile, ty0 = L.v0 + (int)blockIdx.y * kStatTile;
    if (tx0 >= L.h1 || ty0 >= L.v1) return;
    const int tw = min(kStatTile, L.h1 - tx0), th = min(kStatTile, L.v1 - ty0);
    const int win = g.win, half = win >> 1, n = win * win, nz = n + 2, items = nz * (nz + 1) / 2 - 1;
    const int dw = tw + 2 * half, dh = th + 2 * half;
    for (int i = tid; i < dw * dh; i += kThreads) {
        const int r = i / dw, c = i - r * dw;
        const int y = clampi(ty0 - half + r, 0, g.h - 1), x = clampi(tx0 - half + c, 0, g.w - 1);
        buf[r * kStatPitch + c] = (uint16_t)dgd[(size_t)y * dgd_stride + x];
    }
    for (int i = tid; i < kStatTile * kStatTile; i += kThreads) {
        const int r = i / kStatTile, c = i % kStatTile;
        buf[(kStatRowsD + r) * kStatPitch + c] = r < th && c < tw ? (uint16_t)src[(size_t)(ty0 + r) * src_stride + tx0 + c] : 0;
        buf[(kStatRowsD + kStatTile + r) * kStatPitch + c] = 1;
    }
    __syncthreads();
    int off_a[kStatItemsPerLane], off_b[kStatItemsPerLane];
    uint32_t acc[kStatItemsPerLane];
#pragma unroll
    for (int q = 0; q < kStatItemsPerLane; q++) {
        const int item = tid + kThreads * q;
        int k = 0, rem = item < items ? item : 0;
        while (rem >= nz - k) rem -= nz - k, k++;
        const int l = k + rem;
        // Z index -> LDS offset of its value at pixel (0, 0): window index = horizontal offset * win + vertical offset
        off_a[q] = k < n ? (k % win) * kStatPitch + k / win : (kStatRowsD + (k - n) * kStatTile) * kStatPitch;
        off_b[q] = l < n ? (l % win) * kStatPitch + l / win : (kStatRowsD + (l - n) * kStatTile) * kStatPitch;
        acc[q] = 0;
    }
    for (int i = 0; i < th; i++)
        for (int j = 0; j < tw; j++) {
            const int at = i * kStatPitch + j;
#pragma unroll
            for (int q = 0; q < kStatItemsPerLane; q++) acc[q] += (uint32_t)buf[off_a[q] + at] * (uint32_t)buf[off_b[q] + at];
        }
#pragma unroll
    for (int q = 0; q < kStatItemsPerLane; q++) {
        const int item = tid + kThreads * q;
        if (item < items) atomicAdd(&raw[(size_t)(g.base + u) * kRawStride + item], (unsigned long long)acc[q]);
    }
}

// The integer epilogue of one unit: avg, then M, H and the unrestored SSE from the raw sums.  Every raw sum is below 2^20 * 384^2 < 2^38.
__global__ __launch_bounds__(kThreads) void lr_stats_finish_kernel(const unsigned long long* __restrict__ raw_all, PlaneGeom g, int bd, int64_t* __restrict__ M,
                                                               int64_t* __restrict__ H, int32_t* __restrict__ avg_out, int64_t* __restrict__ sse_none)
{
    const int u = blockIdx.x, unit = g.base + u;
    const Limits L = unit_limits(g, u);
    const int64_t N = (int64_t)(L.h1 - L.h0) * (L.v1 - L.v0);
    const int n = g.win * g.win, nz = n + 2, c = n >> 1;
    const unsigned long long* raw = raw_all + (size_t)unit * kRawStride;
    const int64_t avg = (int64_t)(raw[tri_index(c, n + 1, nz)] / (unsigned long long)N);
    const int64_t sx = (int64_t)raw[tri_index(n, n + 1, nz)];
    const int64_t div = bd == 10 ? 4 : 1;
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) {
        const int k = i / n, l = i - k * n;
        const int64_t hr = (int64_t)raw[tri_index(min(k, l), max(k, l), nz)];
        const int64_t sk = (int64_t)raw[tri_index(k, n + 1, nz)], sl = (int64_t)raw[tri_index(l, n + 1, nz)];
        H[(size_t)unit * SVTHIP_WIENER_STATS_H + i] = (hr - avg * (sk + sl) + N * avg * avg) / div;   // C division: towards zero
        if (l == 0) M[(size_t)unit * SVTHIP_WIENER_STATS_M + k] = ((int64_t)raw[tri_index(k, n, nz)] - avg * sk - avg * sx + N * avg * avg) / div;
    }
    if (threadIdx.x == 0) {
        avg_out[unit] = (int32_t)avg;
        sse_none[unit] = (int64_t)raw[tri_index(n, n, nz)] - 2 * (int64_t)raw[tri_index(c, n, nz)] + (int64_t)raw[tri_index(c, c, nz)];
    }
}

// ---------------------------------------------------------------- solve: one lane per unit, the reference's order of operations on int64
__device__ inline int64_t abs64(int64_t v) { return v < 0 ? -v : v; }
__device__ inline int wrap_index(int i, int win) { return i >= (win >> 1) + 1 ? win - 1 - i : i; }

__device__ bool linsolve(int n, int64_t* A, int stride, int64_t* b, int32_t* x)
{
    for (int k = 0; k < n - 1; k++) {
        for (int i = n - 1; i > k; i--)
            if (abs64(A[(i - 1) * stride + k]) < abs64(A[i * stride + k])) {
                for (int j = 0; j < n; j++) {
                    const int64_t c = A[i * stride + j];
                    A[i * stride + j] = A[(i - 1) * stride + j];
                    A[(i - 1) * stride + j] = c;
                }
                const int64_t c = b[i];
                b[i] = b[i - 1];
                b[i - 1] = c;
            }
        for (int i = k; i < n - 1; i++) {
            if (A[k * stride + k] == 0) return false;
            const int64_t c = A[(i + 1) * stride + k], cd = A[k * stride + k];
            for (int j = 0; j < n; j++) A[(i + 1) * stride + j] -= c / 256 * A[k * stride + j] / cd * 256;
            b[i + 1] -= c * b[k] / cd;
        }
    }
    for (int i = n - 1; i >= 0; i--) {
        if (A[i * stride + i] == 0) return false;
        int64_t c = 0;
        for (int j = i + 1; j <= n - 1; j++) c += A[i * stride + j] * x[j] / kTapScale;
        x[i] = (int32_t)(kTapScale * (b[i] - c) / A[i * stride + i]);
    }
    return true;
}

// which 0: b fixed, a updated (update_a_sep_sym); 1: a fixed, b updated (update_b_sep_sym)
__device__ void update_sep_sym(int win, const int64_t* M, const int64_t* H, int32_t* a, int32_t* b, int which)
{
    const int win2 = win * win, h1 = (win >> 1) + 1, e = h1 - 1;
    int64_t A[4] = {0, 0, 0, 0}, B[16];
    int32_t S[7];
    for (int i = 0; i < 16; i++) B[i] = 0;
    for (int i = 0; i < win; i++)
        for (int j = 0; j < win; j++) {
            if (which == 0)
                A[wrap_index(j, win)] += M[i * win + j] * b[i] / kTapScale;
            else
                A[wrap_index(i, win)] += M[i * win + j] * a[j] / kTapScale;
        }
    for (int i = 0; i < win; i++)
        for (int j = 0; j < win; j++)
            for (int k = 0; k < win; k++)
                for (int l = 0; l < win; l++) {
                    if (which == 0)
                        B[wrap_index(l, win) * h1 + wrap_index(k, win)] += H[j * win * win2 + i * win + k * win2 + l] * b[i] / kTapScale * b[j] / kTapScale;
                    else
                        B[wrap_index(j, win) * h1 + wrap_index(i, win)] += H[i * win * win2 + j * win + k * win2 + l] * a[k] / kTapScale * a[l] / kTapScale;
                }
    for (int i = 0; i < e; i++) A[i] -= A[e] * 2 + B[i * h1 + e] - 2 * B[e * h1 + e];
    for (int i = 0; i < e; i++)
        for (int j = 0; j < e; j++) B[i * h1 + j] -= 2 * (B[i * h1 + e] + B[e * h1 + j] - 2 * B[e * h1 + e]);
    if (!linsolve(e, B, h1, A, S)) return;
    S[e] = (int32_t)kTapScale;
    for (int i = h1; i < win; i++) {
        S[i] = S[win - 1 - i];
        S[e] = (int32_t)((uint32_t)S[e] - 2u * (uint32_t)S[i]);
    }
    int32_t* out = which == 0 ? a : b;
    for (int i = 0; i < win; i++) out[i] = S[i];
}

__device__ void finalize_filter(int win, const int32_t* f, int16_t* fi)
{
    const int half = win >> 1;
    for (int i = 0; i < 8; i++) fi[i] = 0;
    for (int i = 0; i < half; i++) {
        const int64_t dividend = (int32_t)((uint32_t)f[i] * (uint32_t)kFiltStep), divisor = kTapScale;
        fi[i] = (int16_t)(dividend < 0 ? (dividend - divisor / 2) / divisor : (dividend + divisor / 2) / divisor);
    }
    if (win == 7) {
        for (int p = 0; p < 3; p++) fi[p] = (int16_t)clampi(fi[p], tap_min(p), tap_max(p));
    } else {
        fi[2] = (int16_t)clampi(fi[1], tap_min(2), tap_max(2));
        fi[1] = (int16_t)clampi(fi[0], tap_min(1), tap_max(1));
        fi[0] = 0;
    }
    fi[6] = fi[0], fi[5] = fi[1], fi[4] = fi[2];
    fi[3] = (int16_t)(-2 * (fi[0] + fi[1] + fi[2]));
}

__device__ int64_t filter_score(int win, const int64_t* M, const int64_t* H, const int16_t* vf, const int16_t* hf)
{
    const int off = (7 - win) >> 1, win2 = win * win;
    int16_t a[7], b[7];
    int32_t ab[49];
    a[3] = b[3] = kFiltStep;
    for (int i = 0; i < 3; i++) {
        a[i] = a[6 - i] = vf[i];
        b[i] = b[6 - i] = hf[i];
        a[3] -= 2 * vf[i];
        b[3] -= 2 * hf[i];
    }
    for (int k = 0; k < win; k++)
        for (int l = 0; l < win; l++) ab[k * win + l] = a[l + off] * b[k + off];
    int64_t P = 0, Q = 0;
    for (int k = 0; k < win2; k++) {
        P += ab[k] * M[k] / kFiltStep / kFiltStep;
        for (int l = 0; l < win2; l++) Q += ab[k] * H[k * win2 + l] * ab[l] / kFiltStep / kFiltStep / kFiltStep / kFiltStep;
    }
    const int c = win2 >> 1;
    return (Q - 2 * P) - (H[c * win2 + c] - 2 * M[c]);
}

__global__ __launch_bounds__(64) void lr_solve_kernel(const int64_t* __restrict__ M_all, const int64_t* __restrict__ H_all, uint32_t unit_begin, uint32_t unit_end, int win,
                                int16_t* __restrict__ taps, int32_t* __restrict__ rejected)
{
    const uint32_t unit = unit_begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (unit >= unit_end) return;
    const int64_t* M = M_all + (size_t)unit * SVTHIP_WIENER_STATS_M;
    const int64_t* H = H_all + (size_t)unit * SVTHIP_WIENER_STATS_H;
    const int init[7] = {kTapMid[0], kTapMid[1], kTapMid[2], kFiltStep - 2 * (kTapMid[0] + kTapMid[1] + kTapMid[2]), kTapMid[2], kTapMid[1], kTapMid[0]};
    const int off = (7 - win) >> 1;
    int32_t a[7], b[7];
    for (int i = 0; i < win; i++) a[i] = b[i] = (int32_t)(kTapScale / kFiltStep) * init[i + off];
    for (int iter = 1; iter < kNumIters; iter++) {
        update_sep_sym(win, M, H, a, b, 0);
        update_sep_sym(win, M, H, a, b, 1);
    }
    int16_t vf[8], hf[8];
    finalize_filter(win, a, vf);
    finalize_filter(win, b, hf);
    for (int i = 0; i < 8; i++) taps[(size_t)unit * 16 + i] = vf[i], taps[(size_t)unit * 16 + 8 + i] = hf[i];
    rejected[unit] = filter_score(win, M, H, vf, hf) > 0;
}

// ---------------------------------------------------------------- the unit filter: one workgroup = 32 columns of one stripe of one unit
// The stripe's rows with three above and three below sit in LDS; the stripe rule is applied while loading (EbRestoration.c:346-467): rows
// above the stripe come from the deblocked plane (rows y0-2, y0-2, y0-1) unless the stripe is the picture's first, rows below it (y1,
// y1+1, y1+1, clamped to the last row) unless it is the last; everything else is the CDEF'd plane with clamped coordinates.
constexpr int kFiltCols = 32;
constexpr int kFiltRows = 64 + 6;
constexpr int kFiltPitch = kFiltCols + 8;   // 6 halo columns, padded

template <typename T, bool WRITE>
__global__ __launch_bounds__(kThreads) void lr_filter_kernel(const T* __restrict__ cdef, uint32_t cdef_stride, const T* __restrict__ dbk, uint32_t dbk_stride,
                                                         const T* __restrict__ src, uint32_t src_stride, T* __restrict__ out, uint32_t out_stride,
                                                         PlaneGeom g, int bd, const uint8_t* __restrict__ taps_base, size_t taps_stride,
                                                         const uint8_t* __restrict__ flag_base, size_t flag_stride,
                                                         unsigned long long* __restrict__ sse, uint32_t* __restrict__ refused)
{
    __shared__ uint16_t in[kFiltRows * kFiltPitch];
    __shared__ uint16_t mid[kFiltRows * kFiltCols];
    __shared__ unsigned long long block_sse;
    const int u = blockIdx.z, unit = g.base + u, tid = threadIdx.x;
    // trial: flag = skip this unit; write: flag = the unit's restoration type
    const int flag = flag_base ? flag_base[(size_t)unit * flag_stride] : (WRITE ? SVTHIP_RESTORE_WIENER : 0);
    if (!WRITE && flag) return;
    const Limits L = unit_limits(g, u);
    const int x0 = L.h0 + (int)blockIdx.x * kFiltCols;
    if (x0 >= L.h1) return;
    const int tw = min(kFiltCols, L.h1 - x0);
    const int sh = 64 >> g.ss, off = 8 >> g.ss;
    const int k = (L.v0 + off) / sh + (int)blockIdx.y;          // the stripe's index in the picture
    const int y0 = max(k * sh - off, L.v0), y1 = min((k + 1) * sh - off, L.v1);
    if (y0 >= L.v1) return;
    const int nrows = y1 - y0;
    if (WRITE && flag != SVTHIP_RESTORE_WIENER) {
        if (flag == SVTHIP_RESTORE_NONE) {
            for (int i = tid; i < nrows * kFiltCols; i += kThreads) {
                const int r = i / kFiltCols, c = i % kFiltCols;
                if (c < tw) out[(size_t)(y0 + r) * out_stride + x0 + c] = cdef[(size_t)(y0 + r) * cdef_stride + x0 + c];
            }
        } else if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
            atomicAdd(refused, 1u);
        }
        return;
    }
    const bool above = y0 != 0, below = (k + 1) * sh - off < g.h;
    const int16_t* taps = reinterpret_cast<const int16_t*>(taps_base + (size_t)unit * taps_stride);
    int fv[7], fh[7];
#pragma unroll
    for (int i = 0; i < 7; i++) fv[i] = taps[i], fh[i] = taps[8 + i];
    const int cols = tw + 6;
    for (int i = tid; i < (nrows + 6) * cols; i += kThreads) {
        const int r = i / cols, c = i - r * cols;
        const int y = y0 - 3 + r, x = clampi(x0 - 3 + c, 0, g.w - 1);
        uint16_t v;
        if (y < y0 && above)
            v = (uint16_t)dbk[(size_t)max(y, y0 - 2) * dbk_stride + x];
        else if (y >= y1 && below)
            v = (uint16_t)dbk[(size_t)min(min(y, y1 + 1), g.h - 1) * dbk_stride + x];
        else
            v = (uint16_t)cdef[(size_t)clampi(y, 0, g.h - 1) * cdef_stride + x];
        in[r * kFiltPitch + c] = v;
    }
    if (tid == 0) block_sse = 0;
    __syncthreads();
    // horizontal: 7 taps plus the centre sample, round_0 = 3, clamped to [0, WIENER_CLAMP_LIMIT(3, bd))
    const int lim0 = (1 << (bd + 1 + 7 - 3)) - 1;
    for (int i = tid; i < (nrows + 6) * kFiltCols; i += kThreads) {
        const int r = i / kFiltCols, c = i % kFiltCols;
        if (c >= tw) continue;
        const uint16_t* p = &in[r * kFiltPitch + c];
        int sum = ((int)p[3] << 7) + (1 << (bd + 6));
#pragma unroll
        for (int t = 0; t < 7; t++) sum += (int)p[t] * fh[t];
        mid[r * kFiltCols + c] = (uint16_t)clampi((sum + 4) >> 3, 0, lim0);
    }
    __syncthreads();
    // vertical: round_1 = 11 with the negative offset, clipped to the pixel range
    const int top = (1 << bd) - 1;
    unsigned long long acc = 0;
    for (int i = tid; i < nrows * kFiltCols; i += kThreads) {
        const int r = i / kFiltCols, c = i % kFiltCols;
        if (c >= tw) continue;
        const uint16_t* p = &mid[r * kFiltCols + c];
        int sum = ((int)p[3 * kFiltCols] << 7) - (1 << (bd + 10));
#pragma unroll
        for (int t = 0; t < 7; t++) sum += (int)p[t * kFiltCols] * fv[t];
        const int v = clampi((sum + 1024) >> 11, 0, top);
        if (WRITE) {
            out[(size_t)(y0 + r) * out_stride + x0 + c] = (T)v;
        } else {
            const int d = v - (int)src[(size_t)(y0 + r) * src_stride + x0 + c];
            acc += (unsigned long long)(d * d);
        }
    }
    if (!WRITE) {
        if (acc) atomicAdd(&block_sse, acc);
        __syncthreads();
        if (tid == 0 && block_sse) atomicAdd(&sse[unit], block_sse);
    }
}

// ---------------------------------------------------------------- the walk (EbRestorationPick.c:1257-1366) as a state machine
__device__ inline void move_tap(int16_t* f, int p, int d)
{
    f[p] = (int16_t)(f[p] + d);
    f[6 - p] = (int16_t)(f[6 - p] + d);
    f[3] = (int16_t)(f[3] - 2 * d);
}

// after the attempts on tap p end: the next tap -- or, when a minus move was accepted, past the last one (`if (skip) break;` leaves the
// loop over p) --, then the other filter, then the next step
__device__ inline void next_tap(svthip_wiener_walk_state& S)
{
    const int p = S.skip ? 3 : S.tap + 1;
    S.dir = 0, S.skip = 0;
    if (p < 3) {
        S.tap = (int8_t)p;
        return;
    }
    S.tap = S.first_tap;
    if (S.filt == 0) {
        S.filt = 1;
        return;
    }
    S.filt = 0;
    S.step >>= 1;
    if (S.step == 0) S.done = 1;
}

// from the position (step, filt, tap, dir): apply the move of the next trial, or mark the walk done
__device__ inline void advance(svthip_wiener_walk_state& S)
{
    while (!S.done) {
        int16_t* f = S.taps + (S.filt ? 0 : 8);
        const int p = S.tap, s = S.step;
        if (S.dir == 0) {
            if (f[p] - s >= tap_min(p)) {
                move_tap(f, p, -s);
                return;
            }
            if (!S.skip) {
                S.dir = 1;
                continue;
            }
        } else if (f[p] + s <= tap_max(p)) {
            move_tap(f, p, s);
            return;
        }
        next_tap(S);
    }
}

__global__ __launch_bounds__(64) void lr_walk_init_kernel(svthip_wiener_walk_state* __restrict__ state, const int16_t* __restrict__ taps, const int32_t* __restrict__ rejected,
                                    uint32_t unit_begin, uint32_t unit_end, int win)
{
    const uint32_t unit = unit_begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (unit >= unit_end) return;
    svthip_wiener_walk_state S{};
    const bool rej = rejected && rejected[unit];
    S.err = rej ? INT64_MAX : 0;
    for (int i = 0; i < 16; i++) S.taps[i] = taps[(size_t)unit * 16 + i];
    S.step = 4;
    S.first_tap = S.tap = (int8_t)((7 - win) >> 1);
    S.done = rej;
    state[unit] = S;
}

__global__ __launch_bounds__(64) void lr_walk_step_kernel(svthip_wiener_walk_state* __restrict__ state, const int64_t* __restrict__ trial_sse, uint32_t unit_begin,
                                    uint32_t unit_end, int32_t* __restrict__ pending)
{
    const uint32_t unit = unit_begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (unit >= unit_end) return;
    svthip_wiener_walk_state S = state[unit];
    if (S.done) return;
    const int64_t e = trial_sse[unit];
    S.n_trials++;
    if (!S.started) {
        S.started = 1;
        S.err = e;
    } else {
        int16_t* f = S.taps + (S.filt ? 0 : 8);
        const int s = S.step, d = S.dir == 0 ? -s : s;
        if (e > S.err) {   // a tie is accepted
            move_tap(f, S.tap, -d);
            if (S.dir == 0 && !S.skip)
                S.dir = 1;
            else
                next_tap(S);
        } else {
            S.err = e;
            if (S.dir == 0) S.skip = 1;
            if (s != 4) next_tap(S);   // at step 4 an accepted move repeats in the same direction
        }
    }
    advance(S);
    state[unit] = S;
    if (!S.done && pending) atomicAdd(pending, 1);
}

__global__ __launch_bounds__(64) void lr_search_output_kernel(const svthip_wiener_walk_state* __restrict__ state, const int64_t* __restrict__ sse_none, uint32_t unit_begin,
                                        uint32_t unit_end, int64_t* __restrict__ sse, int16_t* __restrict__ taps, int32_t* __restrict__ n_trials)
{
    const uint32_t unit = unit_begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (unit >= unit_end) return;
    const svthip_wiener_walk_state S = state[unit];
    const bool rej = S.err == INT64_MAX;
    sse[2 * (size_t)unit] = sse_none[unit];
    sse[2 * (size_t)unit + 1] = S.err;
    for (int i = 0; i < 16; i++) taps[(size_t)unit * 16 + i] = rej ? (int16_t)0 : S.taps[i];
    n_trials[unit] = S.n_trials;
}

template <typename T>
const T* plane_ptr(const void* p) { return static_cast<const T*>(p); }

}  // namespace

// ---------------------------------------------------------------- host side
uint32_t lr_unit_geometry(uint32_t width, uint32_t height, const uint32_t unit_size[3], uint32_t unit_base[4], int32_t* limits)
{
    uint32_t n = 0;
    for (int p = 0; p < 3; p++) {
        const PlaneGeom g = plane_geom(width, height, unit_size, p);
        unit_base[p] = (uint32_t)g.base;
        for (int i = 0; i < g.nx * g.ny; i++, n++)
            if (limits) {
                const Limits L = unit_limits(g, i);
                limits[4 * n] = L.h0, limits[4 * n + 1] = L.h1, limits[4 * n + 2] = L.v0, limits[4 * n + 3] = L.v1;
            }
    }
    unit_base[3] = n;
    return n;
}

uint32_t lr_walk_max_trials(int win)
{
    // the first trial; step 4: per filter and tap one failing minus attempt, then at most (max - min) / 4 plus moves; steps 2 and 1: a minus
    // and a plus attempt per filter and tap
    uint32_t at4 = 0;
    const int off = (7 - win) >> 1;
    for (int p = off; p < 3; p++) at4 += 1 + (tap_max(p) - tap_min(p)) / 4;
    return 1 + 2 * at4 + 2 * 2 * 2 * (3 - off);
}

LrWorkspace lr_workspace(uint32_t n_units)
{
    LrWorkspace w;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    w.raw = take((size_t)n_units * kRawStride * 8);
    w.M = take((size_t)n_units * SVTHIP_WIENER_STATS_M * 8);
    w.H = take((size_t)n_units * SVTHIP_WIENER_STATS_H * 8);
    w.sse_none = take((size_t)n_units * 8);
    w.trial_sse = take((size_t)n_units * 8);
    w.state = take((size_t)n_units * sizeof(svthip_wiener_walk_state));
    w.start_taps = take((size_t)n_units * 32);
    w.avg = take((size_t)n_units * 4);
    w.rejected = take((size_t)n_units * 4);
    w.total = at;
    return w;
}

template <typename T>
static hipError_t stats_t(const svthip_lr_picture& pic, int ps, int pe, int bd, void* raw, int64_t* M, int64_t* H, int32_t* avg, int64_t* sse_none,
                          hipStream_t s)
{
    for (int p = ps; p < pe; p++) {
        const PlaneGeom g = plane_geom(pic.width, pic.height, pic.unit_size, p);
        const int n = g.nx * g.ny, tiles = (g.unit * 3 / 2 + kStatTile - 1) / kStatTile;
        auto* r = static_cast<unsigned long long*>(raw);
        hipError_t e = hipMemsetAsync(r + (size_t)g.base * kRawStride, 0, (size_t)n * kRawStride * 8, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(lr_stats_kernel<T>, dim3(tiles, tiles, n), dim3(kThreads), 0, s, plane_ptr<T>(pic.cdef[p]), pic.cdef_stride[p],
                           plane_ptr<T>(pic.source[p]), pic.source_stride[p], g, r);
        hipLaunchKernelGGL(lr_stats_finish_kernel, dim3(n), dim3(kThreads), 0, s, r, g, bd, M, H, avg, sse_none);
    }
    return hipGetLastError();
}

hipError_t launch_lr_stats(const svthip_lr_picture& pic, int ps, int pe, int bd, void* raw, int64_t* M, int64_t* H, int32_t* avg, int64_t* sse_none,
                           hipStream_t s)
{
    return bd > 8 ? stats_t<uint16_t>(pic, ps, pe, bd, raw, M, H, avg, sse_none, s) : stats_t<uint8_t>(pic, ps, pe, bd, raw, M, H, avg, sse_none, s);
}

hipError_t launch_lr_solve(const int64_t* M, const int64_t* H, uint32_t unit_begin, uint32_t unit_end, int win, int16_t* taps, int32_t* rejected,
                           hipStream_t s)
{
    if (unit_end == unit_begin) return hipSuccess;
    hipLaunchKernelGGL(lr_solve_kernel, dim3((unit_end - unit_begin + 63) / 64), dim3(64), 0, s, M, H, unit_begin, unit_end, win, taps, rejected);
    return hipGetLastError();
}

template <typename T, bool WRITE>
static hipError_t filter_t(const svthip_lr_picture& pic, void* const out[3], const uint32_t out_stride[3], int ps, int pe, int bd, const void* taps,
                           size_t taps_stride, const uint8_t* flag, size_t flag_stride, int64_t* sse, uint32_t* refused, hipStream_t s)
{
    for (int p = ps; p < pe; p++) {
        const PlaneGeom g = plane_geom(pic.width, pic.height, pic.unit_size, p);
        const int n = g.nx * g.ny, max_side = g.unit * 3 / 2, sh = 64 >> g.ss;
        if (!WRITE) {
            hipError_t e = hipMemsetAsync(sse + g.base, 0, (size_t)n * 8, s);
            if (e != hipSuccess) return e;
        }
        // a unit of up to 1.5 unit sizes starts on a stripe boundary (or at row 0) and so meets at most ceil(1.5 unit / stripe) + 1 stripes
        hipLaunchKernelGGL((lr_filter_kernel<T, WRITE>), dim3((max_side + kFiltCols - 1) / kFiltCols, (max_side + sh - 1) / sh + 1, n), dim3(kThreads), 0, s,
                           plane_ptr<T>(pic.cdef[p]), pic.cdef_stride[p], plane_ptr<T>(pic.deblocked[p]), pic.deblocked_stride[p],
                           plane_ptr<T>(pic.source[p]), pic.source_stride[p], WRITE ? static_cast<T*>(out[p]) : nullptr, WRITE ? out_stride[p] : 0u, g, bd,
                           static_cast<const uint8_t*>(taps), taps_stride, flag, flag_stride, reinterpret_cast<unsigned long long*>(sse), refused);
    }
    return hipGetLastError();
}

hipError_t launch_lr_trial(const svthip_lr_picture& pic, int ps, int pe, int bd, const void* taps, size_t taps_stride, const uint8_t* skip,
                           size_t skip_stride, int64_t* sse, hipStream_t s)
{
    return bd > 8 ? filter_t<uint16_t, false>(pic, nullptr, nullptr, ps, pe, bd, taps, taps_stride, skip, skip_stride, sse, nullptr, s)
                  : filter_t<uint8_t, false>(pic, nullptr, nullptr, ps, pe, bd, taps, taps_stride, skip, skip_stride, sse, nullptr, s);
}

hipError_t launch_lr_filter_frame(const svthip_lr_picture& pic, void* const out[3], const uint32_t out_stride[3], int ps, int pe, int bd,
                                  const uint8_t* unit_type, const int16_t* taps, uint32_t* refused, hipStream_t s)
{
    return bd > 8 ? filter_t<uint16_t, true>(pic, out, out_stride, ps, pe, bd, taps, 32, unit_type, 1, nullptr, refused, s)
                  : filter_t<uint8_t, true>(pic, out, out_stride, ps, pe, bd, taps, 32, unit_type, 1, nullptr, refused, s);
}

hipError_t launch_lr_walk_init(svthip_wiener_walk_state* state, const int16_t* taps, const int32_t* rejected, uint32_t unit_begin, uint32_t unit_end,
                               int win, hipStream_t s)
{
    if (unit_end == unit_begin) return hipSuccess;
    hipLaunchKernelGGL(lr_walk_init_kernel, dim3((unit_end - unit_begin + 63) / 64), dim3(64), 0, s, state, taps, rejected, unit_begin, unit_end, win);
    return hipGetLastError();
}

hipError_t launch_lr_walk_step(svthip_wiener_walk_state* state, const int64_t* trial_sse, uint32_t unit_begin, uint32_t unit_end, int32_t* pending,
                               hipStream_t s)
{
    if (pending) {
        hipError_t e = hipMemsetAsync(pending, 0, 4, s);
        if (e != hipSuccess) return e;
    }
    if (unit_end == unit_begin) return hipSuccess;
    hipLaunchKernelGGL(lr_walk_step_kernel, dim3((unit_end - unit_begin + 63) / 64), dim3(64), 0, s, state, trial_sse, unit_begin, unit_end, pending);
    return hipGetLastError();
}

hipError_t launch_lr_search_output(const svthip_wiener_walk_state* state, const int64_t* sse_none, uint32_t unit_begin, uint32_t unit_end, int64_t* sse,
                                   int16_t* taps, int32_t* n_trials, hipStream_t s)
{
    if (unit_end == unit_begin) return hipSuccess;
    hipLaunchKernelGGL(lr_search_output_kernel, dim3((unit_end - unit_begin + 63) / 64), dim3(64), 0, s, state, sse_none, unit_begin, unit_end, sse, taps,
                       n_trials);
    return hipGetLastError();
}

}  // namespace svthip
