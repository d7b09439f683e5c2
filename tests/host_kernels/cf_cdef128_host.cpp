// tests/host_kernels/cf_cdef128_host.cpp -- the CDEF kernels for grids with 128-wide blocks on the host (tests/test_cdef128_kernels_host.py):
// the strength search per 64x64 quadrant into the workspace, the merge into the tables, the pick with its copies; every kernel over the
// grid its launch code uses, the workspace and the grid of exactly the sizes the entries ask for.
// usage: cf_cdef128_host <in> <out>.  in: int32 hd[4] = w, h, bd, base_qindex; double lambda; the deblocked and the source plane of each
// plane in turn, the skip map and the sb_type map (one byte per 4x4 luma cell, width / 4 a row).
#include "hip_on_host.h"

#include "cf_cdef_kernels.h"
using namespace svthip;

template <typename T> static void run(FILE* in, FILE* out, int w, int h, int bd, int qindex, double lambda)
{
    std::vector<T> dbk[3], src[3];
    for (int p = 0; p < 3; p++) { const size_t n = (size_t)(w >> (p > 0)) * (h >> (p > 0)); dbk[p] = rd<T>(in, n); src[p] = rd<T>(in, n); }
    const size_t cells = (size_t)(w / 4) * (h / 4);
    std::vector<uint8_t> skip = rd<uint8_t>(in, cells), sb_type = rd<uint8_t>(in, cells);
    std::vector<svthip_lf_mi> mi(cells);
    for (size_t i = 0; i < cells; i++) mi[i] = svthip_lf_mi{sb_type[i], 0, 0, 0};
    const int nhfb = cdef_fbs(w), nfb = nhfb * cdef_fbs(h);
    CdefPlanes<T> P;
    for (int p = 0; p < 3; p++) {
        P.dbk[p] = dbk[p].data(), P.src[p] = src[p].data(), P.out[p] = nullptr;
        P.dbk_stride[p] = P.src_stride[p] = P.out_stride[p] = (uint32_t)(w >> (p > 0));
    }
    P.w = w, P.h = h, P.skip = skip.data(), P.skip_stride = (uint32_t)(w / 4);
    std::vector<uint64_t> work((size_t)nfb * 3 * 64, 0x7777), mse((size_t)2 * nfb * 64, 0x7777);
    std::vector<uint8_t> counted(nfb, 9);
    launch(cdef_search_grid(w, h), kThreads, [&] {
        cdef_search_kernel<T, true>(P, 3 + (qindex >> 6), bd - 8, (unsigned long long*)work.data(), counted.data(), nullptr, nullptr);
    });
    launch(cdef_search_grid(w, h), kCdefMergeThreads, [&] {
        cdef_merge128_kernel((const unsigned long long*)work.data(), mi.data(), (uint32_t)(w / 4), w, h, bd - 8, (unsigned long long*)mse.data(), counted.data());
    });
    svthip_cdef_result res;
    memset(&res, 0xff, sizeof(res));
    std::vector<int8_t> fbs(nfb, 77);
    launch(dim3(1), kCdefPickThreads, [&] {
        cdef_pick128_kernel((const unsigned long long*)mse.data(), counted.data(), nfb, lambda, 3 + (qindex >> 6), &res, fbs.data(), mi.data(), (uint32_t)(w / 4), nhfb);
    });
    wr(out, mse), wr(out, counted);
    fwrite(&res, sizeof(res), 1, out);
    wr(out, fbs);
}

int main(int argc, char** argv)
{
    FILE* in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE* out = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    int32_t hd[4];
    double lambda;
    if (!in || !out || fread(hd, 4, 4, in) != 4 || fread(&lambda, 8, 1, in) != 1) return 2;
    if (hd[2] > 8)
        run<uint16_t>(in, out, hd[0], hd[1], hd[2], hd[3], lambda);
    else
        run<uint8_t>(in, out, hd[0], hd[1], hd[2], hd[3], lambda);
    fclose(out);
    return 0;
}
