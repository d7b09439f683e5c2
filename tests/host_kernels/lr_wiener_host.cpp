// tests/host_kernels/lr_wiener_host.cpp -- the Wiener kernels on the host (tests/test_lr_kernels_host.py): statistics, solve, the SSE of one
// trial per unit and the frame filter of one assignment, every kernel over the grid its launch code uses.
// usage: lr_wiener_host <in> <out>; exit code 3 when a unit was refused
#include "hip_on_host.h"

#include "lr_wiener_kernels.h"
using namespace svthip;

template <typename T> static int run(FILE* in, FILE* out, int w, int h, int bd, const uint32_t* unit, int n_units)
{
    std::vector<T> cdef[3], dbk[3], src[3], res[3];
    for (int p = 0; p < 3; p++) { const size_t n = (size_t)(w >> (p > 0)) * (h >> (p > 0)); cdef[p] = rd<T>(in, n); dbk[p] = rd<T>(in, n); src[p] = rd<T>(in, n); res[p].assign(n, 7); }
    std::vector<int16_t> trial_taps = rd<int16_t>(in, 16 * n_units), frame_taps = rd<int16_t>(in, 16 * n_units);
    std::vector<uint8_t> types = rd<uint8_t>(in, n_units);
    std::vector<unsigned long long> raw((size_t)n_units * kRawStride, 0), sse(n_units, 0);
    std::vector<int64_t> M((size_t)n_units * 49, -1), H((size_t)n_units * 2401, -1), none(n_units, -1);
    std::vector<int32_t> avg(n_units, -1), rej(n_units, -1);
    std::vector<int16_t> start(16 * n_units, -1);
    uint32_t refused = 0;
    for (int p = 0; p < 3; p++) {
        const PlaneGeom g = plane_geom(w, h, unit, p);
        const int n = g.nx * g.ny;
        launch(lr_stats_grid(g), kThreads, [&] { lr_stats_kernel<T>(cdef[p].data(), g.w, src[p].data(), g.w, g, raw.data()); });
        launch(unit_grid(g), kThreads, [&] { lr_stats_finish_kernel(raw.data(), g, bd, M.data(), H.data(), avg.data(), none.data()); });
        launch(lane_grid(n), 64, [&] { lr_solve_kernel(M.data(), H.data(), g.base, g.base + n, g.win, start.data(), rej.data()); });
        launch(lr_filter_grid(g), kThreads, [&] {
            lr_filter_kernel<T, false>(cdef[p].data(), g.w, dbk[p].data(), g.w, src[p].data(), g.w, nullptr, 0, g, bd, (const uint8_t*)trial_taps.data(), 32,
                                       nullptr, 0, sse.data(), nullptr, 0);
        });
        launch(lr_filter_grid(g), kThreads, [&] {
            lr_filter_kernel<T, true>(cdef[p].data(), g.w, dbk[p].data(), g.w, src[p].data(), g.w, res[p].data(), g.w, g, bd, (const uint8_t*)frame_taps.data(), 32,
                                      types.data(), 1, nullptr, &refused, 0);
        });
    }
    wr(out, M), wr(out, H), wr(out, none), wr(out, avg), wr(out, rej), wr(out, start), wr(out, sse);
    for (int p = 0; p < 3; p++) wr(out, res[p]);
    return (int)refused;
}

int main(int argc, char** argv)
{
    FILE* in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE* out = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    int32_t hd[8];
    if (!in || !out || fread(hd, 4, 8, in) != 8) return 2;
    const uint32_t unit[3] = {(uint32_t)hd[3], (uint32_t)hd[4], (uint32_t)hd[5]};
    const int refused = hd[2] > 8 ? run<uint16_t>(in, out, hd[0], hd[1], hd[2], unit, hd[6]) : run<uint8_t>(in, out, hd[0], hd[1], hd[2], unit, hd[6]);
    fclose(out);
    return refused ? 3 : 0;
}
