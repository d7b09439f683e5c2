// tests/host_kernels/film_grain_host.cpp -- the __device__ arithmetic and index geometry of svt-av1-1_amd/csrc/fg_grain_kernels.h compiled
// by g++ behind hip_on_host.h and run over one picture: the scaling tables, every template draw through the parity masks, the
// autoregressive filters on the kernel's own schedule (fg_ar_schedule_step: luma, Cb and Cr rows skewed and overlapped, with the sliding
// register window; within a step the lanes run from the last to the first, so a chroma lane never sees luma of its own step), and the frame pass unit by unit.  The three source and the three destination planes are allocated exactly
// w x h and w/2 x h/2 with NO border and a stride equal to the width, so under -fsanitize=address a read or write outside the interior
// ends the run.  LDS, barriers and the vector loads are the GPU test's business.
//   usage: film_grain_host IN OUT      IN: int32 width, height, bit depth, vector flag; svthip_film_grain_params; the Y, Cb, Cr planes
//   OUT: the table block (int16), then the Y, Cb, Cr planes with grain
#include "hip_on_host.h"

#include "fg_grain_kernels.h"

using namespace svthip;

template <int LAG>
static void tables(const FgParams& P, int16_t* out)
{
    constexpr int LANES = 256;   // FG_TABLES_THREADS
    for (int k = 0; k < 3 * 256; k++) {
        const int p = P.csfl ? 0 : k >> 8;
        out[FG_TAB_SCALING + k] = (int16_t)fg_scaling_entry(P.point_x[p], P.point_y[p], P.num_points[p], k & 255);
    }
    for (int lane = 0; lane < LANES; lane++) fg_fill_templates(P, out, lane, LANES);
    if constexpr (LAG > 0) {
        std::vector<FgArLane<LAG>> st(LANES);
        for (int s = 0; s < fg_ar_steps<LAG>(); s++)
            for (int lane = LANES - 1; lane >= 0; lane--) fg_ar_schedule_step<LAG>(P, out, lane, s, st[lane]);   // chroma lanes before luma lanes
    } else if (P.num_points[0]) {
        const int lo = fg_grain_min(P.bit_depth), hi = fg_grain_max(P.bit_depth);
        for (int q = 0; q < 2; q++)
            for (int i = 3; P.num_points[1 + q] && i < FG_CHROMA_H; i++)
                for (int j = 3; j < FG_CHROMA_W - 3; j++) {
                    FgArLane<0> st;
                    fg_ar_step<0>(out + (q ? FG_TAB_CR : FG_TAB_CB), FG_CHROMA_W, i, j, P.coeffs[1 + q], P.ar_shift, lo, hi,
                                  P.coeffs[1 + q][0] * fg_luma_mean(out + FG_TAB_LUMA, i, j), st);
                }
    }
}

template <typename T>
static void frame(const FgParams& P, uint32_t w, uint32_t h, bool vec, const std::vector<uint8_t> src[3], std::vector<uint8_t> dst[3], const int16_t* tab)
{
    const void* s[3] = {src[0].data(), src[1].data(), src[2].data()};
    void* d[3] = {dst[0].data(), dst[1].data(), dst[2].data()};
    const uint32_t stride[3] = {w, w / 2, w / 2};
    FgFrame f = fg_make_frame(P, s, stride, d, stride, w, h, tab);
    if (!vec) f.vec_luma = f.vec_chroma = 0;
    for (uint32_t uy = 0; uy < (h + 15) / 16 * 8; uy++)     // the kernel's grid, the units outside the picture included
        for (uint32_t ux = 0; ux < (w + 255) / 256 * 32; ux++) fg_apply_unit<T>(f, tab + FG_TAB_SCALING, ux, uy);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    const std::vector<int32_t> hd = rd<int32_t>(fi, 4);
    const uint32_t w = (uint32_t)hd[0], h = (uint32_t)hd[1];
    const int bd = hd[2], bytes = bd > 8 ? 2 : 1;
    const std::vector<uint8_t> raw = rd<uint8_t>(fi, sizeof(svthip_film_grain_params));
    svthip_film_grain_params params;
    memcpy(&params, raw.data(), sizeof(params));
    std::vector<uint8_t> src[3], dst[3];
    for (int p = 0; p < 3; p++) {
        const size_t n = (size_t)(w >> (p > 0)) * (h >> (p > 0)) * bytes;
        src[p] = rd<uint8_t>(fi, n);
        dst[p].assign(n, 0xAA);
    }
    fclose(fi);

    const FgParams P = fg_narrow(params, bd);
    std::vector<int16_t> tab(FG_TAB_INT16);
    switch (P.lag) {
    case 0: tables<0>(P, tab.data()); break;
    case 1: tables<1>(P, tab.data()); break;
    case 2: tables<2>(P, tab.data()); break;
    default: tables<3>(P, tab.data()); break;
    }
    if (bd == 8) frame<uint8_t>(P, w, h, hd[3] != 0, src, dst, tab.data()); else frame<uint16_t>(P, w, h, hd[3] != 0, src, dst, tab.data());

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    wr(fo, tab), wr(fo, dst[0]), wr(fo, dst[1]), wr(fo, dst[2]);
    fclose(fo);
    return 0;
}
