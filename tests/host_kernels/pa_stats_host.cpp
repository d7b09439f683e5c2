// tests/host_kernels/pa_stats_host.cpp -- the __device__ arithmetic and index geometry of svt-av1-1_amd/csrc/pa_stats_kernels.h compiled by
// g++ behind hip_on_host.h and run over one picture: every leaf, pyramid node and output of the block statistics in the order the kernel's
// lanes take them, the homogeneity of every SB with the picture's flags, and every histogram region.  The planes are allocated with exactly
// the border the entries require (68 samples around the luma plane, 16 around the 1/16 plane, none around chroma), so under
// -fsanitize=address a read outside them ends the run.  Lane mapping, LDS and barriers are the GPU test's business.
//   usage: pa_stats_host IN OUT      IN: int32 width, height, sub_precision; the unpadded luma, Cb, Cr planes
//   OUT: y_mean, variance, cb_mean, cr_mean, var_of_var, homogeneous, picture, histogram, region_intensity, average_intensity
#include "hip_on_host.h"

#include "pa_stats_kernels.h"

using namespace svthip;

// a plane of w x h samples with `pad` replicated samples around it, and not a byte more
static std::vector<uint8_t> padded(const std::vector<uint8_t>& src, int src_stride, int step, int w, int h, int pad)
{
    const int stride = w + 2 * pad;
    std::vector<uint8_t> out((size_t)stride * (h + 2 * pad));
    for (int Y = 0; Y < h + 2 * pad; Y++)
        for (int X = 0; X < stride; X++)
            out[(size_t)Y * stride + X] = src[(size_t)(min(max(Y - pad, 0), h - 1) * step) * src_stride + min(max(X - pad, 0), w - 1) * step];
    return out;
}

template <int SUB>
static void block_stats(const std::vector<uint8_t>& full, const std::vector<uint8_t> chroma[2], uint32_t w, uint32_t h, std::vector<uint8_t>& y_mean,
                        std::vector<uint16_t>& variance, std::vector<uint8_t> c_mean[2])
{
    const uint32_t stride = w + 136, cstride = w / 2, n_sb = ((w + 63) / 64) * ((h + 63) / 64);
    for (uint32_t sb = 0; sb < n_sb; sb++) {
        uint32_t mean[85], mean_sq[85], cmean[2][21], x0, y0;
        const bool complete = pa_sb_origin(w, h, sb, &x0, &y0);
        for (uint32_t lane = 0; lane < 64; lane++)
            pa_leaf<SUB, true>(full.data() + (size_t)(68 + y0 + 8 * (lane >> 3)) * stride + 68 + x0 + 8 * (lane & 7), stride, &mean[21 + lane], &mean_sq[21 + lane]);
        for (uint32_t lane = 0; lane < 32; lane++) {
            uint32_t m = 0, unused;
            const uint32_t cl = lane & 15;
            if (complete) pa_leaf<SUB, false>(chroma[lane >> 4].data() + (size_t)((y0 >> 1) + 8 * (cl >> 2)) * cstride + (x0 >> 1) + 8 * (cl & 3), cstride, &m, &unused);
            cmean[lane >> 4][5 + cl] = m;
        }
        for (int level = 2; level >= 0; level--)
            for (int k = 0; k < 1 << (2 * level); k++) pa_pyramid_node(mean, level, k), pa_pyramid_node(mean_sq, level, k);
        for (int p = 0; p < 2; p++) {
            for (int k = 0; k < 4; k++) pa_pyramid_node(cmean[p], 1, k);
            pa_chroma_top(cmean[p]);
        }
        for (int i = 0; i < 85; i++) y_mean[sb * 85 + i] = pa_mean_out(mean[i]), variance[sb * 85 + i] = pa_variance_out(mean[i], mean_sq[i]);
        for (int p = 0; p < 2; p++)
            for (int i = 0; i < 21; i++) c_mean[p][sb * 21 + i] = pa_mean_out(cmean[p][i]);
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> hd = rd<int32_t>(f, 3);
    const uint32_t w = (uint32_t)hd[0], h = (uint32_t)hd[1], n_sb = ((w + 63) / 64) * ((h + 63) / 64);
    const std::vector<uint8_t> luma = rd<uint8_t>(f, (size_t)w * h);
    std::vector<uint8_t> chroma[2] = {rd<uint8_t>(f, (size_t)w * h / 4), rd<uint8_t>(f, (size_t)w * h / 4)};
    fclose(f);
    const std::vector<uint8_t> full = padded(luma, (int)w, 1, (int)w, (int)h, 68), sixteenth = padded(luma, (int)w, 4, (int)(w >> 2), (int)(h >> 2), 16);

    std::vector<uint8_t> y_mean(n_sb * 85), c_mean[2] = {std::vector<uint8_t>(n_sb * 21), std::vector<uint8_t>(n_sb * 21)}, homogeneous(n_sb);
    std::vector<uint16_t> variance(n_sb * 85);
    if (hd[2]) block_stats<1>(full, chroma, w, h, y_mean, variance, c_mean); else block_stats<0>(full, chroma, w, h, y_mean, variance, c_mean);

    std::vector<uint64_t> var_of_var(n_sb * 4);
    std::vector<uint32_t> picture(4), acc(3, 0);
    for (uint32_t sb = 0; sb < n_sb; sb++) {
        uint32_t x0, y0;
        const bool complete = pa_sb_origin(w, h, sb, &x0, &y0);
        homogeneous[sb] = pa_sb_homogeneity(&variance[sb * 85], complete, &var_of_var[sb * 4]);
        acc[0] += variance[sb * 85];
        if (complete) acc[2]++, acc[1] += variance[sb * 85] < 5;
    }
    pa_picture_flags(acc[0], acc[1], acc[2], n_sb, picture.data());

    std::vector<uint32_t> histogram(16 * 3 * 256), region_intensity(16 * 3), average_intensity(3);
    uint64_t total[3] = {0, 0, 0};
    for (uint32_t rx = 0; rx < 4; rx++)
        for (uint32_t ry = 0; ry < 4; ry++)
            for (int plane = 0; plane < 3; plane++) {
                const PaHistRegion R = pa_hist_region(w, h, plane, rx, ry);
                const uint32_t stride = plane ? w / 2 : (w >> 2) + 32;
                const uint8_t* origin = plane ? chroma[plane - 1].data() : sixteenth.data() + (size_t)16 * stride + 16;
                uint32_t bins[256] = {0}, sum = 0;
                for (uint32_t i = 0; i < R.cols * R.rows; i++) {
                    const uint32_t j = i / R.cols, v = origin[(size_t)(R.y0 + j * R.step) * stride + R.x0 + (i - j * R.cols) * R.step];
                    bins[v]++, sum += v;
                }
                const size_t o = (rx * 4 + ry) * 3 + plane;
                for (int b = 0; b < 256; b++) histogram[o * 256 + b] = (1u + bins[b]) << 4;
                region_intensity[o] = pa_region_intensity(R, plane, sum);
                total[plane] += sum << 4;
            }
    for (int plane = 0; plane < 3; plane++) average_intensity[plane] = pa_average_intensity(total[plane], w, h, plane);

    f = fopen(argv[2], "wb");
    if (!f) return 2;
    wr(f, y_mean), wr(f, variance), wr(f, c_mean[0]), wr(f, c_mean[1]), wr(f, var_of_var), wr(f, homogeneous), wr(f, picture), wr(f, histogram);
    wr(f, region_intensity), wr(f, average_intensity);
    fclose(f);
    return 0;
}
