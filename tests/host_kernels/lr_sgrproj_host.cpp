// tests/host_kernels/lr_sgrproj_host.cpp -- the self-guided kernels on the host (tests/test_lr_sgr_kernels_host.py): the box filter over the
// planes for every set, the whole search with its records, the SSE of the search's filter, the frame filter of one assignment (both unit
// filters, as the frame entry runs them) and, with hd[7] set, the solve alone; every kernel over the grid its launch code uses.
// usage: lr_sgrproj_host <in> <out>; exit code 3 when a unit was refused
#include "hip_on_host.h"

#include "lr_sgrproj_kernels.h"
#include "lr_wiener_kernels.h"
using namespace svthip;

template <typename T> static int run(FILE* in, FILE* out, int w, int h, int bd, const uint32_t* unit, int n_units)
{
    std::vector<T> cdef[3], dbk[3], src[3], res[3];
    for (int p = 0; p < 3; p++) { const size_t n = (size_t)(w >> (p > 0)) * (h >> (p > 0)); cdef[p] = rd<T>(in, n); dbk[p] = rd<T>(in, n); src[p] = rd<T>(in, n); res[p].assign(n, 7); }
    std::vector<int16_t> taps = rd<int16_t>(in, 16 * n_units);
    std::vector<uint8_t> types = rd<uint8_t>(in, n_units);
    std::vector<int32_t> usgr = rd<int32_t>(in, 4 * n_units);
    const size_t jobs = (size_t)n_units * kSgrParams;
    std::vector<int64_t> sums(jobs * 5, -1), err(jobs, -1), fsums(3 * 16 * 4, 0);
    std::vector<int32_t> size(jobs, -1), ep(jobs, -1), ntr(jobs, -1), xq(jobs * 2, -1), start(jobs * 2, -1), fin(jobs * 2, -1), sgrproj(4 * n_units, -1);
    std::vector<svthip_sgrproj_detail> detail(jobs);
    std::vector<unsigned long long> sse(n_units, 0);
    std::vector<int32_t> dump;
    uint32_t refused = 0;
    for (int p = 0; p < 3; p++) {
        const PlaneGeom g = plane_geom(w, h, unit, p);
        const int n = g.nx * g.ny;
        const size_t plane = (size_t)g.w * g.h;
        // the plane entry, every set: sums of flt and flt^2; the samples minus u for sets 0, 12, 15
        for (int e = 0; e < kSgrParams; e++) {
            std::vector<int32_t> f0(plane, -7), f1(plane, -7);
            launch(sgr_box_grid(g), kThreads, [&] {
                sgr_box_kernel<T, false>(cdef[p].data(), g.w, (const T*)nullptr, 0, g, bd, e, e + 1, f0.data(), f1.data(), g.w, nullptr, nullptr);
            });
            for (size_t i = 0; i < plane; i++) {
                if (sgr_r(e, 0)) fsums[(p * 16 + e) * 4] += f0[i], fsums[(p * 16 + e) * 4 + 1] += (int64_t)f0[i] * f0[i]; else if (f0[i] != -7) abort();
                if (sgr_r(e, 1)) fsums[(p * 16 + e) * 4 + 2] += f1[i], fsums[(p * 16 + e) * 4 + 3] += (int64_t)f1[i] * f1[i]; else if (f1[i] != -7) abort();
            }
            if (e == 0 || e == 12 || e == 15)
                for (int k = 0; k < 2; k++)
                    for (size_t i = 0; i < plane; i++) dump.push_back(sgr_r(e, k) ? (k ? f1 : f0)[i] - ((int32_t)cdef[p][i] << 4) : 0);
        }
        // the search
        std::vector<int16_t> f16(plane * kSgrParams * 2, 0x7777);
        const size_t j0 = (size_t)g.base * kSgrParams;
        launch(lane_grid(n * kSgrParams), 64, [&] { sgr_search_init_kernel(g, sums.data(), size.data(), ep.data()); });
        launch(sgr_box_grid(g), kThreads, [&] {
            sgr_box_kernel<T, true>(cdef[p].data(), g.w, src[p].data(), g.w, g, bd, 0, kSgrParams, nullptr, nullptr, 0, f16.data(), (unsigned long long*)sums.data());
        });
        launch(lane_grid(n * kSgrParams), 64, [&] {
            sgr_solve_kernel(sums.data() + j0 * 5, size.data() + j0, ep.data() + j0, n * kSgrParams, xq.data() + j0 * 2, start.data() + j0 * 2);
        });
        launch(sgr_walk_grid(g), kThreads, [&] {
            sgr_walk_kernel<T>(cdef[p].data(), g.w, src[p].data(), g.w, g, f16.data(), start.data(), fin.data(), err.data(), ntr.data());
        });
        launch(lane_grid(n), 64, [&] {
            sgr_pick_kernel(sums.data(), xq.data(), start.data(), fin.data(), err.data(), ntr.data(), g.base, g.base + n, sgrproj.data(), detail.data());
        });
        // the SSE of the search's filter, then the frame filter with the run's types
        launch(sgr_filter_grid(g), kThreads, [&] {
            sgr_filter_kernel<T, false>(cdef[p].data(), g.w, dbk[p].data(), g.w, src[p].data(), g.w, nullptr, 0, g, bd, sgrproj.data(), nullptr, sse.data(), nullptr);
        });
        launch(sgr_filter_grid(g), kThreads, [&] {
            sgr_filter_kernel<T, true>(cdef[p].data(), g.w, dbk[p].data(), g.w, (const T*)nullptr, 0, res[p].data(), g.w, g, bd, usgr.data(), types.data(), nullptr,
                                       &refused);
        });
        launch(lr_filter_grid(g), kThreads, [&] {
            lr_filter_kernel<T, true>(cdef[p].data(), g.w, dbk[p].data(), g.w, (const T*)nullptr, 0, res[p].data(), g.w, g, bd, (const uint8_t*)taps.data(), 32,
                                      types.data(), 1, nullptr, &refused, 1);
        });
    }
    wr(out, fsums), wr(out, dump);
    fwrite(detail.data(), sizeof(svthip_sgrproj_detail), detail.size(), out);
    wr(out, sgrproj), wr(out, sse);
    for (int p = 0; p < 3; p++) wr(out, res[p]);
    return (int)refused;
}

int main(int argc, char** argv)
{
    FILE* in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE* out = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    int32_t hd[8];
    if (!in || !out || fread(hd, 4, 8, in) != 8) return 2;
    int refused = 0;
    if (hd[7]) {   // the solve alone: hd[6] jobs
        const int n = hd[6];
        std::vector<int64_t> sums = rd<int64_t>(in, 5 * n);
        std::vector<int32_t> size = rd<int32_t>(in, n), ep = rd<int32_t>(in, n), xq(2 * n, -1), xqd(2 * n, -1);
        launch(lane_grid(n), 64, [&] { sgr_solve_kernel(sums.data(), size.data(), ep.data(), n, xq.data(), xqd.data()); });
        wr(out, xq), wr(out, xqd);
    } else {
        const uint32_t unit[3] = {(uint32_t)hd[3], (uint32_t)hd[4], (uint32_t)hd[5]};
        refused = hd[2] > 8 ? run<uint16_t>(in, out, hd[0], hd[1], hd[2], unit, hd[6]) : run<uint8_t>(in, out, hd[0], hd[1], hd[2], unit, hd[6]);
    }
    fclose(out);
    return refused ? 3 : 0;
}
