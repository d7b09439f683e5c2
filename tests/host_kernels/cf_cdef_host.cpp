// tests/host_kernels/cf_cdef_host.cpp -- the CDEF kernels on the host (tests/test_cdef_kernels_host.py): the strength search of a picture
// with its directions, the pick on the search's own tables, the frame filter of the runs given; with hd[5] == 1 the pick alone on tables
// given, with hd[5] == 2 dist_8x8 on block pairs; every kernel over the grid its launch code uses.
// usage: cf_cdef_host <in> <out>.  in: int32 hd[8] = w, h, bd, base_qindex, runs, mode, n, 0; double lambda; then the mode's data.
#include "hip_on_host.h"

#include "cf_cdef_kernels.h"
using namespace svthip;

static void pick(const std::vector<uint64_t>& mse, const std::vector<uint8_t>& counted, int nfb, double lambda, int qindex, FILE* out)
{
    svthip_cdef_result res;
    memset(&res, 0xff, sizeof(res));
    std::vector<int8_t> fbs(nfb, 77);
    launch(dim3(1), kCdefPickThreads, [&] { cdef_pick_kernel((const unsigned long long*)mse.data(), counted.data(), nfb, lambda, 3 + (qindex >> 6), &res, fbs.data()); });
    fwrite(&res, sizeof(res), 1, out);
    wr(out, fbs);
}

template <typename T> static void run(FILE* in, FILE* out, int w, int h, int bd, int qindex, int runs, double lambda)
{
    std::vector<T> dbk[3], src[3], res[3];
    for (int p = 0; p < 3; p++) { const size_t n = (size_t)(w >> (p > 0)) * (h >> (p > 0)); dbk[p] = rd<T>(in, n); src[p] = rd<T>(in, n); }
    std::vector<uint8_t> skip = rd<uint8_t>(in, (size_t)(w / 4) * (h / 4));
    const int nfb = cdef_fbs(w) * cdef_fbs(h);
    CdefPlanes<T> P;
    for (int p = 0; p < 3; p++) {
        P.dbk[p] = dbk[p].data(), P.src[p] = src[p].data(), P.out[p] = nullptr;
        P.dbk_stride[p] = P.src_stride[p] = P.out_stride[p] = (uint32_t)(w >> (p > 0));
    }
    P.w = w, P.h = h, P.skip = skip.data(), P.skip_stride = (uint32_t)(w / 4);
    std::vector<uint64_t> mse((size_t)2 * nfb * 64, 0x7777);
    std::vector<uint8_t> counted(nfb, 9);
    std::vector<int32_t> dirs((size_t)nfb * 64, -7), vars((size_t)nfb * 64, -7);
    launch(cdef_search_grid(w, h), kThreads, [&] {
        cdef_search_kernel<T>(P, 3 + (qindex >> 6), bd - 8, (unsigned long long*)mse.data(), counted.data(), dirs.data(), vars.data());
    });
    wr(out, mse), wr(out, counted), wr(out, dirs), wr(out, vars);
    pick(mse, counted, nfb, lambda, qindex, out);
    for (int r = 0; r < runs; r++) {
        svthip_cdef_result rr;
        if (fread(&rr, sizeof(rr), 1, in) != 1) abort();
        std::vector<int8_t> fbs = rd<int8_t>(in, nfb);
        for (int p = 0; p < 3; p++) res[p].assign(dbk[p].size(), 7), P.out[p] = res[p].data();
        launch(cdef_frame_grid(w, h, 3), kThreads, [&] { cdef_frame_kernel<T>(P, 0, bd - 8, &rr, fbs.data()); });
        for (int p = 0; p < 3; p++) wr(out, res[p]);
    }
}

int main(int argc, char** argv)
{
    FILE* in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE* out = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    int32_t hd[8];
    double lambda;
    if (!in || !out || fread(hd, 4, 8, in) != 8 || fread(&lambda, 8, 1, in) != 1) return 2;
    if (hd[5] == 1) {          // the pick alone: hd[6] fbs
        const int nfb = hd[6];
        std::vector<uint64_t> mse = rd<uint64_t>(in, (size_t)2 * nfb * 64);
        std::vector<uint8_t> counted = rd<uint8_t>(in, nfb);
        pick(mse, counted, nfb, lambda, hd[3], out);
    } else if (hd[5] == 2) {   // dist_8x8: hd[6] pairs
        const int n = hd[6];
        std::vector<uint16_t> dst = rd<uint16_t>(in, (size_t)n * 64), src = rd<uint16_t>(in, (size_t)n * 64);
        std::vector<uint64_t> d(n, 0x7777);
        launch(lane_grid(n), 64, [&] { cdef_dist_8x8_kernel(dst.data(), src.data(), n, hd[2] - 8, (unsigned long long*)d.data()); });
        wr(out, d);
    } else if (hd[2] > 8) {
        run<uint16_t>(in, out, hd[0], hd[1], hd[2], hd[3], hd[4], lambda);
    } else {
        run<uint8_t>(in, out, hd[0], hd[1], hd[2], hd[3], hd[4], lambda);
    }
    fclose(out);
    return 0;
}
