// tests/host_kernels/lr_finish_host.cpp -- the restoration-decision kernel on the host (tests/test_lr_finish_kernels_host.py): the kernel body
// of lr_finish_kernels.h over the grid its launch code uses, one lane per workgroup doing every phase in order, on the tables of one case.
// Also: the direct bit counts on an exhaustive (ref, v) grid per symbol class, for the test to compare with the restatement's.
// usage: lr_finish_host <in> <out>; exit code 3 when a unit was refused
//   in:  int32 hd[16] = rdmult, wiener_cost[2], sgrproj_cost[2], switchable_cost[3], unit_base[4], plane_start, plane_end, want_best_rtype, 0
//        then wiener_sse[n][2] int64, taps[n][16] int16, sgr_sse[n] int64, sgrproj[n][4] int32
//   out: unit_type[n] u8, best_rtype[n][4] u8, result[3], refused u32, then the counts: per class n * n bytes [ref][v]
#include "hip_on_host.h"

#include "lr_finish_kernels.h"
#include "lr_sgrproj_kernels.h"
#include "lr_wiener_kernels.h"
using namespace svthip;

// the ranges stated in lr_finish_kernels.h are those of the two search kernels
static_assert(kFinMin[0] == tap_min(0) && kFinMin[1] == tap_min(1) && kFinMin[2] == tap_min(2), "tap minima");
static_assert(kFinN[0] == tap_max(0) - tap_min(0) + 1 && kFinN[1] == tap_max(1) - tap_min(1) + 1 && kFinN[2] == tap_max(2) - tap_min(2) + 1, "tap ranges");
static_assert(kFinMid[0] == kTapMid[0] && kFinMid[1] == kTapMid[1] && kFinMid[2] == kTapMid[2], "default taps");
static_assert(kFinMin[3] == prj_min(0) && kFinMin[4] == prj_min(1) && kFinN[3] == prj_max(0) - prj_min(0) + 1 && kFinN[4] == prj_max(1) - prj_min(1) + 1, "xqd ranges");
static_assert(kFinLutAt[4] + kFinN[4] == kFinLutSize && kFinLutAt[1] == kFinN[0] && kFinLutAt[2] == kFinLutAt[1] + kFinN[1] &&
              kFinLutAt[3] == kFinLutAt[2] + kFinN[2], "table layout");

int main(int argc, char** argv)
{
    FILE* in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE* out = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    int32_t hd[16];
    if (!in || !out || fread(hd, 4, 16, in) != 16) return 2;
    FinishArgs a;
    a.rates.rdmult = hd[0];
    for (int i = 0; i < 2; i++) a.rates.wiener_cost[i] = hd[1 + i], a.rates.sgrproj_cost[i] = hd[3 + i];
    for (int i = 0; i < 3; i++) a.rates.switchable_cost[i] = hd[5 + i];
    for (int i = 0; i < 4; i++) a.unit_base[i] = (uint32_t)hd[8 + i];
    const int ps = hd[12], pe = hd[13];
    a.plane_start = (uint32_t)ps;
    const size_t n = a.unit_base[3];
    // exact sizes, so that an index past a table ends the run under the sanitizer
    std::vector<int64_t> wiener_sse = rd<int64_t>(in, 2 * n);
    std::vector<int16_t> taps = rd<int16_t>(in, 16 * n);
    std::vector<int64_t> sgr_sse = rd<int64_t>(in, n);
    std::vector<int32_t> sgrproj = rd<int32_t>(in, 4 * n);
    std::vector<uint8_t> unit_type(n, 0x5A), best_rtype(4 * n, 0x5A);
    std::vector<svthip_rest_finish_result> result(3);
    memset(result.data(), 0x5A, sizeof(svthip_rest_finish_result) * 3);
    uint32_t refused = 0;
    launch(dim3(pe - ps), kThreads, [&] {
        rest_finish_kernel(a, wiener_sse.data(), taps.data(), sgr_sse.data(), sgrproj.data(), unit_type.data(), hd[14] ? best_rtype.data() : nullptr,
                           result.data(), &refused);
    });
    wr(out, unit_type), wr(out, best_rtype);
    fwrite(result.data(), sizeof(svthip_rest_finish_result), 3, out);
    fwrite(&refused, 4, 1, out);
    for (int c = 0; c < 5; c++) {
        std::vector<uint8_t> counts;
        for (int r = 0; r < kFinN[c]; r++)
            for (int v = 0; v < kFinN[c]; v++) counts.push_back((uint8_t)fin_count_refsubexpfin(c, r, v));
        wr(out, counts);
    }
    fclose(out);
    return refused ? 3 : 0;
}
