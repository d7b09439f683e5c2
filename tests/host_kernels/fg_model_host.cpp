// tests/host_kernels/fg_model_host.cpp -- the __host__ __device__ arithmetic and index geometry of svt-av1-1_amd/csrc/fg_noise_model_kernels.h
// compiled by g++ behind hip_on_host.h and run over one picture: the noise model as its three kernels walk it (every entry's serial sum
// over the staged tiles of the flat blocks, the block sums, then fgm_finish with one lane doing the workgroup's work) and the flat-block
// tables and features.  The six planes and the map are allocated at exactly their size with a stride equal to the width, and every tile
// and block at exactly its size, so under -fsanitize=address a read or write outside ends the run.  What this cannot show -- the lanes'
// division of the work, the barriers, the device's double division and square root -- is what tests/test_fg_model_gpu.py is for.
//   usage: fg_model_host IN OUT     IN: int32 width, height, bit depth; the Y, Cb, Cr data planes; the Y, Cb, Cr denoised planes; the map
//   OUT: svthip_film_grain_noise_state; the tables (doubles); the features of every block; the is_flat bytes
#include "hip_on_host.h"

#include "fg_noise_model_kernels.h"

using namespace svthip;

template <typename T>
static void model(const FgmPicture& P, svthip_film_grain_noise_state* state)
{
    const int nb = P.nbw * P.nbh;
    std::vector<double> obs(3 * FGM_OBS_STRIDE, 0.0);
    std::vector<FgmBlockStats> stats(3 * nb);
    int32_t n_obs[3] = {0, 0, 0};
    const double normalization = (1 << P.bit_depth) - 1, norm2 = normalization * normalization;
    for (int c = 0; c < 3; c++) {
        const int n = FGM_COORDS + (c > 0);
        for (int by = 0; by < P.nbh; by++)
            for (int bx = 0; bx < P.nbw; bx++) {
                if (!P.flat[by * P.nbw + bx]) continue;
                const FgmBlock g = fgm_block(P, c > 0, bx, by);
                const int k = fgm_block_observations(g);
                if (!k) continue;
                n_obs[c] += k;
                std::vector<double> tile(FGM_TILE_DOUBLES);
                fgm_stage<T>(P, c, g, tile.data(), 0, 1);
                int i = 0, j = 0;
                for (int e = 0; fgm_entry(n, e, &i, &j); e++) fgm_observe_block(tile.data(), g, fgm_operand(i), fgm_operand(j), norm2, obs[c * FGM_OBS_STRIDE + e]);
            }
        for (int b = 0; b < nb; b++) {
            if (!P.flat[b] || !fgm_strength_gate(P, c > 0, b % P.nbw, b / P.nbw)) continue;
            int64_t s[3];
            fgm_block_sums<T>(P, c, b % P.nbw, b / P.nbw, 0, 1, s);
            stats[c * nb + b] = fgm_block_stats(P, c, b % P.nbw, b / P.nbw, s);
        }
    }
    std::vector<FgmSolveWork> W(1);
    fgm_finish(P, obs.data(), n_obs, stats.data(), *state, W[0], 0, 1);
}

template <typename T>
static void features(const T* luma, int w, int h, int bd, int nbw, int nb, std::vector<double>& tables, std::vector<svthip_film_grain_flat_block_features>& feat,
                     std::vector<uint8_t>& is_flat)
{
    std::vector<FgmSolveWork> W(1);
    std::vector<double> ata(FGF_PARAMS * FGF_PARAMS);
    fgf_tables(tables.data(), W[0], ata.data(), 0, 1);
    for (int b = 0; b < nb; b++) {
        std::vector<double> blk(FGF_N), fit(FGF_PARAMS);
        fgf_extract<T>(luma, w, h, (uint32_t)w, (b % nbw) * FGM_BLOCK, (b / nbw) * FGM_BLOCK, (double)((1 << bd) - 1), tables.data(), blk.data(), fit.data(), 0, 1);
        double sums[5];
        for (int k = 0; k < 5; k++) sums[k] = fgf_interior_sum(blk.data(), k);
        is_flat[b] = fgf_features(sums, &feat[b]);
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    const std::vector<int32_t> hd = rd<int32_t>(fi, 3);
    const int w = hd[0], h = hd[1], bd = hd[2], bytes = bd > 8 ? 2 : 1;
    std::vector<uint8_t> planes[6];
    for (int p = 0; p < 6; p++) planes[p] = rd<uint8_t>(fi, (size_t)(w >> (p % 3 > 0)) * (h >> (p % 3 > 0)) * bytes);
    FgmPicture P;
    P.w = w, P.h = h, P.bit_depth = bd;
    P.nbw = (w + FGM_BLOCK - 1) / FGM_BLOCK, P.nbh = (h + FGM_BLOCK - 1) / FGM_BLOCK;
    const int nb = P.nbw * P.nbh;
    const std::vector<uint8_t> flat = rd<uint8_t>(fi, nb);
    fclose(fi);
    for (int c = 0; c < 3; c++) P.data[c] = planes[c].data(), P.den[c] = planes[3 + c].data(), P.stride[c] = (uint32_t)(w >> (c > 0));
    P.flat = flat.data();

    std::vector<svthip_film_grain_noise_state> state(1);
    memset(state.data(), 0xAA, sizeof(state[0]));
    std::vector<double> tables(SVTHIP_FILM_GRAIN_FLAT_TABLES_DOUBLES);
    std::vector<svthip_film_grain_flat_block_features> feat(nb);
    std::vector<uint8_t> is_flat(nb);
    if (bd == 8) {
        model<uint8_t>(P, state.data());
        features<uint8_t>(planes[0].data(), w, h, bd, P.nbw, nb, tables, feat, is_flat);
    } else {
        model<uint16_t>(P, state.data());
        features<uint16_t>(reinterpret_cast<const uint16_t*>(planes[0].data()), w, h, bd, P.nbw, nb, tables, feat, is_flat);
    }

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    wr(fo, state), wr(fo, tables), wr(fo, feat), wr(fo, is_flat);
    fclose(fo);
    return 0;
}
