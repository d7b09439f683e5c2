// tests/host_kernels/md_fast_host.cpp -- the __device__ arithmetic and index geometry of svt-av1-1_amd/csrc/md_fast_kernels.h compiled by g++
// behind hip_on_host.h: the quad walk of every lane of a candidate over Y, Cb and Cr (md_fast_lane_sads with the lane count the launch
// picks), the flags and the cost (md_fast_finish), and the buffer walk with PreModeDecision (md_fast_pick_group, its buffers at the stride
// the kernel's LDS columns have).  The six planes are allocated exactly width x height at a stride equal to the width, `shift` bytes into
// their allocations, so under -fsanitize=address a read past the last sample of a plane ends the run: the test puts a source block and a
// prediction tile into the last rows and columns.  The cross-lane sum, the LDS and the vector stores are the GPU test's business.
//   usage: md_fast_host IN OUT
//   IN:  int32 bwidth, bheight, n, src_w, src_h, src_cw, src_ch, pool_w, pool_h, pool_cw, pool_ch, shift, m, n_groups; the source Y, Cb, Cr;
//        the pool Y, Cb, Cr; svthip_md_fast_desc[n]; then for the pick svthip_md_fast_result[m], svthip_md_fast_desc[m],
//        svthip_md_fast_group[n_groups]
//   OUT: svthip_md_fast_result[n], svthip_md_fast_pick[n_groups], int32 refused groups
#include "hip_on_host.h"

#include <memory>

#include "md_fast_kernels.h"

using namespace svthip;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    const std::vector<int32_t> hd = rd<int32_t>(fi, 14);
    const uint32_t bw = (uint32_t)hd[0], bh = (uint32_t)hd[1], n = (uint32_t)hd[2], m = (uint32_t)hd[12], n_groups = (uint32_t)hd[13];
    const size_t shift = (size_t)hd[11];
    const size_t dims[6][2] = {{(size_t)hd[3], (size_t)hd[4]}, {(size_t)hd[5], (size_t)hd[6]}, {(size_t)hd[5], (size_t)hd[6]},
                               {(size_t)hd[7], (size_t)hd[8]}, {(size_t)hd[9], (size_t)hd[10]}, {(size_t)hd[9], (size_t)hd[10]}};
    std::unique_ptr<uint8_t[]> mem[6];   // new[] of exactly shift + width * height bytes: a vector may keep capacity behind its size
    for (int p = 0; p < 6; p++) {
        const std::vector<uint8_t> plane = rd<uint8_t>(fi, dims[p][0] * dims[p][1]);
        mem[p].reset(new uint8_t[shift + plane.size()]);
        memset(mem[p].get(), 0x5A, shift);
        memcpy(mem[p].get() + shift, plane.data(), plane.size());
    }
    const std::vector<svthip_md_fast_desc> desc = rd<svthip_md_fast_desc>(fi, n);
    const std::vector<svthip_md_fast_result> p_result = rd<svthip_md_fast_result>(fi, m);
    const std::vector<svthip_md_fast_desc> p_desc = rd<svthip_md_fast_desc>(fi, m);
    const std::vector<svthip_md_fast_group> groups = rd<svthip_md_fast_group>(fi, n_groups);
    fclose(fi);

    const svthip_inter_planes src = {mem[0].get() + shift, mem[1].get() + shift, mem[2].get() + shift, (uint32_t)dims[0][0], (uint32_t)dims[1][0]};
    const svthip_inter_planes pool = {mem[3].get() + shift, mem[4].get() + shift, mem[5].get() + shift, (uint32_t)dims[3][0], (uint32_t)dims[4][0]};
    std::vector<svthip_md_fast_result> result(n);
    const MdFastArgs A = md_fast_make_args(src, pool, desc.data(), n, bw, bh, result.data());
    const int lanes = md_fast_group_lanes(bw, bh);
    for (uint32_t job = 0; job < n; job++) {
        uint32_t luma = 0, chroma = 0;
        for (int l = 0; l < lanes; l++) {
            uint32_t a, b;
            md_fast_lane_sads(A, desc[job], l, lanes, &a, &b);
            luma += a, chroma += b;
        }
        result[job] = md_fast_finish(desc[job], luma, chroma);
    }

    std::vector<svthip_md_fast_pick> picks(n_groups);
    std::vector<uint64_t> cost((size_t)MD_FAST_BUFFERS * MD_FAST_PICK_THREADS);
    std::vector<uint8_t> cand((size_t)MD_FAST_BUFFERS * MD_FAST_PICK_THREADS), best((size_t)MD_FAST_BUFFERS * MD_FAST_PICK_THREADS);
    int32_t refused = 0;
    for (uint32_t i = 0; i < n_groups; i++) {
        const int column = (int)(i % MD_FAST_PICK_THREADS);
        refused += !md_fast_pick_group(p_result.data(), p_desc.data(), m, groups[i], &cost[column], &cand[column], &best[column],
                                       MD_FAST_PICK_THREADS, &picks[i]);
    }

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    wr(fo, result), wr(fo, picks), wr(fo, std::vector<int32_t>{refused});
    fclose(fo);
    return 0;
}
