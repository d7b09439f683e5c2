// svt-av1-1_amd/csrc/ip_inter_pred.hip
//
// Whole-PU AV1 inter prediction: Y, Cb and Cr of a batch of prediction units of one luma size, each what one call of
// av1_inter_prediction / av1_inter_prediction_hbd writes (Source/Lib/Codec/EbInterPrediction.c:1005-2050 / :2053-).
//
//   expansion  one thread per PU: clamp_mv_to_umv_border_sb for luma (bw, bh, 0, 0) and chroma (bwidth_uv, bheight_uv, 1, 1),
//              integer / fraction split, source and destination offsets, the sub8x8_inter decision (:1044-1127) and its pieces
//              (:1129-1245).  Each PU becomes one job in a uni-list-0 / uni-list-1 / bi list per plane kind (the Cb and Cr jobs of a PU
//              have the same offsets: the two chroma planes share one stride), or up to four chroma pieces.  Slots come from per-list
//              counters in device memory (each in the 16 bytes in front of its list), one atomic per list and workgroup.
//   luma, chroma >= 4x4   the convolution kernels of the per-plane entries (ip_convolve.hip / ip_convolve_mfma.hip) in their counted
//              form (template flag COUNTED): the job count is read from device memory and the grid is sized for n_pu.
//   pieces     2x2 / 2x4 / 4x2 / 2x8 / 8x2 chroma pieces of sub-8x8 blocks: inter_pred_piece_kernel below, one thread per piece and plane,
//              the whole piece in registers (no LDS); filter classes are inputs chosen by the expansion from bwidth_uv / bheight_uv.
// The clamp, the chroma geometry, the job word, the filter rows and the rounding constants are ip_common.h's.
//
// Offsets are 32-bit and the source planes are passed rebased (rebase_samples), so every offset is non-negative.  A PU whose offsets would
// still leave that range (mb_to_*_edge values that do not describe the block's position) is refused like a BI_PRED PU with sub-8x8 chroma:
// nothing is written, the context counts it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svtav1_hip.h"
#include "ip_common.h"
#include "ip_launch.h"

static_assert(sizeof(svthip_inter_pu_desc) == 64, "svthip_inter_pu_desc is 64 bytes (include/svtav1_hip.h)");

namespace svthip {

namespace {

// scratch slot layout: the job lists, each behind a 16-byte slot whose first dword is its length (where the counted convolution kernels
// read it); lists 0-5 hold up to n jobs, the piece list up to 4 n
enum { L_Y0, L_Y1, L_YBI, L_C0, L_C1, L_CBI, L_PIECE, N_LISTS };
constexpr size_t kHeader = 256;
__host__ __device__ inline size_t list_pitch(uint32_t n) { return (size_t)n * 16 + 16; }
__host__ __device__ inline size_t count_offset(int l, uint32_t n) { return kHeader + (size_t)l * list_pitch(n); }
__host__ __device__ inline size_t list_offset(int l, uint32_t n) { return count_offset(l, n) + 16; }

struct ExpandArgs {
    uint32_t ys0, ys1, yd, cs0, cs1, cd;  // strides: reference 0 / 1 / destination, luma and chroma
    int bw, bh, bwu, bhu;
    int64_t ky0, ky1, kc0, kc1;           // rebasing of the source planes, in samples
};

__device__ __forceinline__ void clamp_mv(int mv_row, int mv_col, const svthip_inter_pu_desc& d, int bw, int bh, int ss, int& r, int& c)
{
    clamp_mv_to_umv_border(mv_row, mv_col, d.mb_to_left_edge, d.mb_to_right_edge, d.mb_to_top_edge, d.mb_to_bottom_edge, bw, bh, ss, r, c);
}

// The piece list's own job: like a uni job, but subpel_y sits beside subpel_x, the reference list is named (the pieces of a PU can differ
// in it) and the filters are CLASSES, chosen from bwidth_uv / bheight_uv and not from the piece's own size.
struct PieceJob {
    uint32_t src, dst;
    int sx, sy, list, fxc, fyc;
};
__device__ __forceinline__ uint4 piece_job(uint32_t src, uint32_t dst, int sx, int sy, int list, int fxc, int fyc)
{
    return uint4{src, dst, (uint32_t)(sx | (sy << 4) | (list << 8) | (fxc << 16) | (fyc << 24)), 0u};
}
__device__ __forceinline__ PieceJob decode_piece(uint4 j)
{
    return PieceJob{j.x, j.y, (int)(j.z & 15), (int)((j.z >> 4) & 15), (int)((j.z >> 8) & 1), (int)((j.z >> 16) & 255), (int)((j.z >> 24) & 255)};
}

// Slot allocation for the seven job lists, aggregated per workgroup: each wave's ballots give its lanes' ranks and counts, one thread per
// list adds the workgroup's total with ONE atomic (the seven in parallel), and a lane's slot is the workgroup base + the waves before it
// + its rank.  (Per-wave atomics issued one list after another cost a memory round trip each: 7 in series per wave, measured 21 us for
// 32 640 PUs.)
__device__ __forceinline__ void alloc_slots(uint4* lists, uint32_t n_pu, const bool (&want)[N_LISTS], uint32_t np, uint32_t (&slot)[N_LISTS])
{
    __shared__ uint32_t wave_n[4][N_LISTS], base[4][N_LISTS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint64_t mask[N_LISTS];
#pragma unroll
    for (int l = 0; l < N_LISTS; l++) {
        mask[l] = __ballot(want[l]);
        if (lane == 0) wave_n[wave][l] = (uint32_t)__popcll(mask[l]) * (l == L_PIECE ? np : 1u);
    }
    __syncthreads();
    if (threadIdx.x < N_LISTS) {
        const int l = threadIdx.x;
        const uint32_t total = wave_n[0][l] + wave_n[1][l] + wave_n[2][l] + wave_n[3][l];
        const uint32_t b = total ? atomicAdd(reinterpret_cast<uint32_t*>(lists + count_offset(l, n_pu) / 16), total) : 0u;
        base[0][l] = b;
        base[1][l] = b + wave_n[0][l];
        base[2][l] = b + wave_n[0][l] + wave_n[1][l];
        base[3][l] = b + wave_n[0][l] + wave_n[1][l] + wave_n[2][l];
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < N_LISTS; l++) {
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask[l] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask[l], 0u));
        slot[l] = base[wave][l] + below * (l == L_PIECE ? np : 1u);
    }
}

__global__ void __launch_bounds__(256) inter_pred_expand_kernel(const svthip_inter_pu_desc* __restrict__ desc, uint32_t n_pu, ExpandArgs A,
                                                                uint4* __restrict__ lists, uint32_t* __restrict__ refused,
                                                                uint8_t* __restrict__ refused_rows)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n_pu;
    svthip_inter_pu_desc d;
    if (live) d = desc[i];
    else __builtin_memset(&d, 0, sizeof(d));
    const int dir = d.pred_direction == 2 ? 2 : (d.pred_direction & 1);
    const int fx = (int)((d.interp_filters >> 16) & 3), fy = (int)(d.interp_filters & 3);
    bool ok = live;

    // ---- luma ----
    int sub[2];
    int64_t ysrc[2];
    for (int l = 0; l < 2; l++) {
        int r, c;
        clamp_mv(d.mv[l][0], d.mv[l][1], d, A.bw, A.bh, 0, r, c);
        sub[l] = (c & 15) | ((r & 15) << 4);
        const uint32_t st = l ? A.ys1 : A.ys0;
        ysrc[l] = ((int64_t)d.pu_origin_y + (r >> 4)) * st + (int64_t)d.pu_origin_x + (c >> 4) + (l ? A.ky1 : A.ky0);
        if ((dir == l || dir == 2) && !offset_in_range(ysrc[l])) ok = false;
    }
    const uint32_t ydst = (uint32_t)d.dst_origin_y * A.yd + d.dst_origin_x;

    // ---- chroma: sub-8x8 decision ----
    const bool narrow = A.bw == 4, flat = A.bh == 4;
    bool sub8 = false;
    if (d.has_uv && (narrow || flat)) {
        sub8 = true;
        if (narrow && flat && !d.nb_is_inter[0]) sub8 = false;
        if (flat && !d.nb_is_inter[1]) sub8 = false;
        if (narrow && !d.nb_is_inter[2]) sub8 = false;
    }
    if (sub8 && dir == 2) ok = false;  // assert(!is_compound) in the reference (:1148, :2195)
    const int cx0 = chroma_origin(d.pu_origin_x), cy0 = chroma_origin(d.pu_origin_y);
    const uint32_t cdst = (uint32_t)chroma_origin(d.dst_origin_y) * A.cd + (uint32_t)chroma_origin(d.dst_origin_x);
    int csub[2];
    int64_t csrc[2];
    const bool whole_c = d.has_uv && !sub8;
    for (int l = 0; l < 2; l++) {
        int r, c;
        clamp_mv(d.mv[l][0], d.mv[l][1], d, A.bwu, A.bhu, 1, r, c);
        csub[l] = (c & 15) | ((r & 15) << 4);
        const uint32_t st = l ? A.cs1 : A.cs0;
        csrc[l] = ((int64_t)cy0 + (r >> 4)) * st + cx0 + (c >> 4) + (l ? A.kc1 : A.kc0);
        if (whole_c && (dir == l || dir == 2) && !offset_in_range(csrc[l])) ok = false;
    }
    // pieces: b4 = (bw / 2) x (bh / 2) over the bwidth_uv x bheight_uv block, (row, col) from (row_start, col_start)
    const int b4w = A.bw >> 1, b4h = A.bh >> 1, npx = A.bwu / b4w, npy = A.bhu / b4h;
    uint4 piece[4];
    if (sub8 && ok) {
        const int fxi = interp_filter_class(fx, A.bwu), fyi = interp_filter_class(fy, A.bhu);
#pragma unroll
        for (int py = 0; py < 2; py++)
#pragma unroll
            for (int px = 0; px < 2; px++) {
                if (py >= npy || px >= npx) continue;
                const int row = py - (flat ? 1 : 0), col = px - (narrow ? 1 : 0);
                int mr, mc, list;
                // selects, not indexing: a dynamic index would put the descriptor in scratch memory
                if (row == 0 && col == 0) {
                    mr = dir ? d.mv[1][0] : d.mv[0][0];
                    mc = dir ? d.mv[1][1] : d.mv[0][1];
                    list = d.own_list & 1;
                } else if (row < 0 && col < 0) {
                    mr = d.nb_mv[0][0]; mc = d.nb_mv[0][1]; list = d.nb_list[0] & 1;
                } else if (row < 0) {
                    mr = d.nb_mv[1][0]; mc = d.nb_mv[1][1]; list = d.nb_list[1] & 1;
                } else {
                    mr = d.nb_mv[2][0]; mc = d.nb_mv[2][1]; list = d.nb_list[2] & 1;
                }
                int r, c;
                clamp_mv(mr, mc, d, A.bwu, A.bhu, 1, r, c);
                const int x = px * b4w, y = py * b4h;
                const uint32_t st = list ? A.cs1 : A.cs0;
                const int64_t so = ((int64_t)cy0 + y + (r >> 4)) * st + cx0 + x + (c >> 4) + (list ? A.kc1 : A.kc0);
                if (!offset_in_range(so)) ok = false;
                piece[py * 2 + px] = piece_job((uint32_t)so, cdst + (uint32_t)y * A.cd + (uint32_t)x, c & 15, r & 15, list, fxi, fyi);
            }
    }
    if (live && !ok) {
        atomicAdd(refused, 1u);
        if (refused_rows) refused_rows[i] = 1;   // for a caller inside the library that has to know which (md_ifs.hip)
    }

    // ---- jobs ----
    const uint32_t np = (uint32_t)(npx * npy);
    bool want[N_LISTS];
#pragma unroll
    for (int l = 0; l < 3; l++) {
        want[L_Y0 + l] = ok && dir == l;
        want[L_C0 + l] = ok && whole_c && dir == l;
    }
    want[L_PIECE] = ok && sub8;
    uint32_t slot[N_LISTS];
    alloc_slots(lists, n_pu, want, np, slot);
#pragma unroll
    for (int l = 0; l < 2; l++) {
        if (want[L_Y0 + l])
            lists[list_offset(L_Y0 + l, n_pu) / 16 + slot[L_Y0 + l]] = uni_job((uint32_t)ysrc[l], ydst, sub[l] & 15, sub[l] >> 4, fx, fy);
        if (want[L_C0 + l])
            lists[list_offset(L_C0 + l, n_pu) / 16 + slot[L_C0 + l]] = uni_job((uint32_t)csrc[l], cdst, csub[l] & 15, csub[l] >> 4, fx, fy);
    }
    if (want[L_YBI])
        lists[list_offset(L_YBI, n_pu) / 16 + slot[L_YBI]] = bi_job((uint32_t)ysrc[0], (uint32_t)ysrc[1], ydst, sub[0], sub[1], fx, fy);
    if (want[L_CBI])
        lists[list_offset(L_CBI, n_pu) / 16 + slot[L_CBI]] = bi_job((uint32_t)csrc[0], (uint32_t)csrc[1], cdst, csub[0], csub[1], fx, fy);
    if (want[L_PIECE])
#pragma unroll
        for (int py = 0; py < 2; py++)
#pragma unroll
            for (int px = 0; px < 2; px++)
                if (py < npy && px < npx) lists[list_offset(L_PIECE, n_pu) / 16 + slot[L_PIECE] + (uint32_t)(py * npx + px)] = piece[py * 2 + px];
}

// One chroma piece of PW x PH samples per thread (threads [0, n) Cb, [n, 2n) Cr), single-reference rounding of
// av1_convolve_{2d,x,y,2d_copy}_sr_c / av1_highbd_convolve_*_sr_c (:145-286, :530-700) with get_conv_params_no_round(.., 0, bd):
// hrow8 and the single-reference second_pass_constants of ip_common.h.
template <int PW, int PH, bool HBD>
__global__ void __launch_bounds__(256) inter_pred_piece_kernel(const uint8_t* __restrict__ r0cb, const uint8_t* __restrict__ r0cr, uint32_t s0,
                                                               const uint8_t* __restrict__ r1cb, const uint8_t* __restrict__ r1cr, uint32_t s1,
                                                               uint8_t* __restrict__ dcb, uint8_t* __restrict__ dcr, uint32_t ds,
                                                               const uint4* __restrict__ jobs, int bd)
{
    constexpr int SB = HBD ? 2 : 1;
    const uint32_t n = __builtin_amdgcn_readfirstlane(jobs[-1].x);
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * n) return;
    const bool cr = t >= n;
    const PieceJob j = decode_piece(jobs[cr ? t - n : t]);
    const int sx = j.sx, sy = j.sy, list = j.list;
    const uint8_t* src = list ? (cr ? r1cr : r1cb) : (cr ? r0cr : r0cb);
    const uint32_t stride = list ? s1 : s0;
    uint8_t* dst = (cr ? dcr : dcb) + (size_t)j.dst * SB;

    int im[PH + 7][PW];
    const int rows = sy ? PH + 7 : PH;
    const int64_t base = (int64_t)j.src - (sy ? 3 * (int64_t)stride : 0) - (sx ? 3 : 0);
    uint32_t flo = 0, fhi = 0;
    if (sx) {
        flo = kInterpFilter[j.fxc][sx][0];
        fhi = kInterpFilter[j.fxc][sx][1];
    }
#pragma unroll
    for (int r = 0; r < PH + 7; r++) {
        if (r >= rows) continue;
        const uint8_t* p = src + (base + (int64_t)r * stride) * SB;
        if (HBD) {
            const uint16_t* p16 = reinterpret_cast<const uint16_t*>(p);
            if (sx) {
                int f[8], s[PW + 7];
                unpack_taps(flo, fhi, f);
#pragma unroll
                for (int k = 0; k < PW + 7; k++) s[k] = p16[k];
                const int bias = (sy ? (1 << (bd + 6)) : 0) + 4;
#pragma unroll
                for (int c = 0; c < PW; c++) {
                    int acc = bias;
#pragma unroll
                    for (int k = 0; k < 8; k++) acc += __mul24(f[k], s[c + k]);
                    im[r][c] = acc >> 3;
                }
            } else {
#pragma unroll
                for (int c = 0; c < PW; c++) im[r][c] = p16[c];
            }
        } else if (sx) {
            hrow8<PW>(p, flo, fhi, sy != 0, im[r]);
        } else {
#pragma unroll
            for (int c = 0; c < PW; c++) im[r][c] = p[c];
        }
    }

    const int pix_max = (1 << bd) - 1;
    int g[8];
    const SecondPass K = second_pass_constants(sx, sy, j.fyc, false, bd, g);
    const int c0 = K.c0, shift = K.shift, subtract = K.sub;
#pragma unroll
    for (int y = 0; y < PH; y++)
#pragma unroll
        for (int c = 0; c < PW; c++) {
            int acc = c0;
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (y + k < PH + 7) acc += __mul24(g[k], im[y + k][c]);
            int v = (acc >> shift) - subtract;
            v = min(max(v, 0), pix_max);
            if (HBD) reinterpret_cast<uint16_t*>(dst)[(size_t)y * ds + c] = (uint16_t)v;
            else dst[(size_t)y * ds + c] = (uint8_t)v;
        }
}

template <bool HBD>
hipError_t launch_pieces(int bw, int bh, const uint8_t* r0cb, const uint8_t* r0cr, uint32_t s0, const uint8_t* r1cb, const uint8_t* r1cr, uint32_t s1,
                         uint8_t* dcb, uint8_t* dcr, uint32_t ds, const uint4* jobs, uint32_t max_jobs, int bd, hipStream_t s)
{
    const dim3 grid((uint32_t)((2 * (uint64_t)max_jobs + 255) / 256)), block(256);
#define SVTHIP_PIECES(PW, PH) \
    hipLaunchKernelGGL((inter_pred_piece_kernel<PW, PH, HBD>), grid, block, 0, s, r0cb, r0cr, s0, r1cb, r1cr, s1, dcb, dcr, ds, jobs, bd)
    if (bw == 4 && bh == 4) SVTHIP_PIECES(2, 2);
    else if (bw == 4 && bh == 8) SVTHIP_PIECES(2, 4);
    else if (bw == 8 && bh == 4) SVTHIP_PIECES(4, 2);
    else if (bw == 4) SVTHIP_PIECES(2, 8);
    else SVTHIP_PIECES(8, 2);
#undef SVTHIP_PIECES
    return hipGetLastError();
}

}  // namespace

bool inter_pred_has_pieces(int bw, int bh) { return bw == 4 || bh == 4; }

size_t inter_pred_scratch_bytes(uint32_t n_pu) { return list_offset(L_PIECE, n_pu) + (size_t)4 * n_pu * 16; }

hipError_t launch_inter_pred(const svthip_inter_planes& ref0, const svthip_inter_planes& ref1, const svthip_inter_planes& dst,
                             const svthip_inter_pu_desc* desc, uint32_t n_pu, int bw, int bh, int bd, bool use_mfma, void* scratch,
                             uint32_t* refused, hipStream_t s, uint8_t* refused_rows)
{
    const int SB = bd > 8 ? 2 : 1;
    const int bwu = chroma_side(bw), bhu = chroma_side(bh);
    ExpandArgs A;
    A.ys0 = ref0.y_stride; A.ys1 = ref1.y_stride; A.yd = dst.y_stride;
    A.cs0 = ref0.c_stride; A.cs1 = ref1.c_stride; A.cd = dst.c_stride;
    A.bw = bw; A.bh = bh; A.bwu = bwu; A.bhu = bhu;
    A.ky0 = rebase_samples(bw, bh, ref0.y_stride); A.ky1 = rebase_samples(bw, bh, ref1.y_stride);
    A.kc0 = rebase_samples(bwu, bhu, ref0.c_stride); A.kc1 = rebase_samples(bwu, bhu, ref1.c_stride);
    uint8_t* sc = static_cast<uint8_t*>(scratch);
    // the seven list lengths: one strided memset
    hipError_t e = hipMemset2DAsync(sc + count_offset(0, n_pu), list_pitch(n_pu), 0, sizeof(uint32_t), N_LISTS, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(inter_pred_expand_kernel, dim3((n_pu + 255) / 256), dim3(256), 0, s, desc, n_pu, A, reinterpret_cast<uint4*>(sc), refused, refused_rows);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    auto rb = [SB](const void* p, int64_t k) { return static_cast<const uint8_t*>(p) - k * SB; };
    const uint8_t *y0 = rb(ref0.y, A.ky0), *y1 = rb(ref1.y, A.ky1);
    const uint8_t *cb0 = rb(ref0.cb, A.kc0), *cb1 = rb(ref1.cb, A.kc1), *cr0 = rb(ref0.cr, A.kc0), *cr1 = rb(ref1.cr, A.kc1);
    // per plane kind: list 0, list 1, both (compound)
    auto run = [&](int w, int h, int l0, const uint8_t* p0, uint32_t s0, const uint8_t* p1, uint32_t s1, void* d, uint32_t dsz) -> hipError_t {
        const bool mfma = use_mfma && bd == 8 && convolve_mfma_size_valid(w, h);
        for (int l = 0; l < 3; l++) {
            const ConvolveLaunch L = {l == 1 ? p1 : p0, l == 1 ? s1 : s0, p1, s1, d, dsz, sc + list_offset(l0 + l, n_pu), n_pu, w, h, bd, l == 2, true};
            const hipError_t r = mfma ? launch_convolve_mfma(L, s) : launch_convolve_valu(L, s);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    };
    if ((e = run(bw, bh, L_Y0, y0, ref0.y_stride, y1, ref1.y_stride, dst.y, dst.y_stride)) != hipSuccess) return e;
    if ((e = run(bwu, bhu, L_C0, cb0, ref0.c_stride, cb1, ref1.c_stride, dst.cb, dst.c_stride)) != hipSuccess) return e;
    if ((e = run(bwu, bhu, L_C0, cr0, ref0.c_stride, cr1, ref1.c_stride, dst.cr, dst.c_stride)) != hipSuccess) return e;
    if (inter_pred_has_pieces(bw, bh)) {
        const uint4* pj = reinterpret_cast<const uint4*>(sc + list_offset(L_PIECE, n_pu));
        const uint32_t max_jobs = n_pu * (uint32_t)((bwu / (bw >> 1)) * (bhu / (bh >> 1)));
        uint8_t *dcb = static_cast<uint8_t*>(dst.cb), *dcr = static_cast<uint8_t*>(dst.cr);
        e = bd > 8 ? launch_pieces<true>(bw, bh, cb0, cr0, ref0.c_stride, cb1, cr1, ref1.c_stride, dcb, dcr, dst.c_stride, pj, max_jobs, bd, s)
                   : launch_pieces<false>(bw, bh, cb0, cr0, ref0.c_stride, cb1, cr1, ref1.c_stride, dcb, dcr, dst.c_stride, pj, max_jobs, 8, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace svthip
