// tests/host_kernels/md_ifs_host.cpp -- the __device__ arithmetic and index geometry of svt-av1-1_amd/csrc/md_ifs_kernels.h compiled by g++
// behind hip_on_host.h: the quad walk of every lane of a tile over Y, Cb and Cr (md_ifs_lane_sses with the lane count the launch picks),
// the model and the RDCOST (md_model_rd_finish), the trial descriptors (md_ifs_emit_trial) and the walk (md_ifs_walk).  The six planes are
// allocated exactly width x height at a stride equal to the width, `shift` bytes into their allocations, so under -fsanitize=address a
// read past the last sample of a plane ends the run: the test puts a source block and a prediction tile into the last rows and columns.
// The cross-lane sums and the vector loads and stores are the GPU test's business.
//   usage: md_ifs_host IN OUT
//   IN:  int32 bwidth, bheight, n, src_w, src_h, pool_w, pool_h, shift, quantizer, n_cand, walk, tiles_per_row; the source Y, Cb, Cr; the
//        pool Y, Cb, Cr; svthip_md_model_rd_desc[n]; then for the search svthip_inter_pu_desc[n_cand], svthip_md_ifs_desc[n_cand],
//        svthip_md_model_rd_result[n_cand * trials] (the trials' measurements), uint8 refused[n_cand * trials]
//   OUT: svthip_md_model_rd_result[n], int32 refused tiles; svthip_inter_pu_desc[n_cand * trials], svthip_md_model_rd_desc[n_cand * trials]
//        (the trial descriptors), svthip_md_ifs_result[n_cand], svthip_inter_pu_desc[n_cand] (written back), int32 refused candidates
#include "hip_on_host.h"

#include <memory>

#include "md_ifs_kernels.h"

using namespace svthip;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    const std::vector<int32_t> hd = rd<int32_t>(fi, 12);
    const uint32_t bw = (uint32_t)hd[0], bh = (uint32_t)hd[1], n = (uint32_t)hd[2], n_cand = (uint32_t)hd[9];
    const size_t shift = (size_t)hd[7];
    const int walk = hd[10];
    const size_t dims[6][2] = {{(size_t)hd[3], (size_t)hd[4]}, {(size_t)hd[3] / 2, (size_t)hd[4] / 2}, {(size_t)hd[3] / 2, (size_t)hd[4] / 2},
                               {(size_t)hd[5], (size_t)hd[6]}, {(size_t)hd[5] / 2, (size_t)hd[6] / 2}, {(size_t)hd[5] / 2, (size_t)hd[6] / 2}};
    std::unique_ptr<uint8_t[]> mem[6];   // new[] of exactly shift + width * height bytes: a vector may keep capacity behind its size
    for (int p = 0; p < 6; p++) {
        const std::vector<uint8_t> plane = rd<uint8_t>(fi, dims[p][0] * dims[p][1]);
        mem[p].reset(new uint8_t[shift + plane.size()]);
        memset(mem[p].get(), 0x5A, shift);
        memcpy(mem[p].get() + shift, plane.data(), plane.size());
    }
    const std::vector<svthip_md_model_rd_desc> desc = rd<svthip_md_model_rd_desc>(fi, n);
    const uint32_t trials = md_ifs_walk_trials(walk), n_tiles = n_cand * trials;
    // 16-byte aligned as the entry demands of the device arrays: the descriptors move as 16-byte quarters
    svthip_inter_pu_desc* pu = static_cast<svthip_inter_pu_desc*>(aligned_alloc(16, sizeof(svthip_inter_pu_desc) * (n_cand + 1)));
    svthip_inter_pu_desc* t_pu = static_cast<svthip_inter_pu_desc*>(aligned_alloc(16, sizeof(svthip_inter_pu_desc) * (n_tiles + 1)));
    if (n_cand && fread(pu, sizeof(svthip_inter_pu_desc), n_cand, fi) != n_cand) abort();
    const std::vector<svthip_md_ifs_desc> ifs = rd<svthip_md_ifs_desc>(fi, n_cand);
    const std::vector<svthip_md_model_rd_result> t_result = rd<svthip_md_model_rd_result>(fi, n_tiles);
    const std::vector<uint8_t> t_refused = rd<uint8_t>(fi, n_tiles);
    fclose(fi);

    const svthip_inter_planes src = {mem[0].get() + shift, mem[1].get() + shift, mem[2].get() + shift, (uint32_t)dims[0][0], (uint32_t)dims[1][0]};
    const svthip_inter_planes pool = {mem[3].get() + shift, mem[4].get() + shift, mem[5].get() + shift, (uint32_t)dims[3][0], (uint32_t)dims[4][0]};
    std::vector<svthip_md_model_rd_result> result(n);
    uint32_t refused_tiles = 0;
    const MdModelRdArgs M = md_model_rd_make_args(src, pool, desc.data(), n, bw, bh, (int16_t)hd[8], result.data(), &refused_tiles);
    const int lanes = md_fast_group_lanes(bw, bh);
    for (uint32_t job = 0; job < n; job++) {
        memset(&result[job], 0, sizeof(result[job]));
        if (!md_model_rd_desc_valid(desc[job])) {
            refused_tiles++;
            continue;
        }
        uint32_t sums[3] = {0, 0, 0};
        for (int l = 0; l < lanes; l++) {
            uint32_t part[3];
            md_ifs_lane_sses(M, desc[job], l, lanes, part);
            for (int k = 0; k < 3; k++) sums[k] += part[k];
        }
        result[job] = md_model_rd_finish(desc[job], sums, (uint32_t)(M.log2_qw + 2 + M.log2_h), M.qstep);
    }

    std::vector<svthip_md_model_rd_desc> t_desc(n_tiles);
    std::vector<svthip_md_ifs_result> found(n_cand);
    uint32_t refused = 0;
    MdIfsArgs A;
    A.pu = pu, A.ifs = ifs.data(), A.result = found.data(), A.n = n_cand;
    A.t_pu = t_pu, A.t_desc = t_desc.data(), A.t_result = t_result.data(), A.t_refused = t_refused.data();
    A.refused = &refused;
    A.tiles_per_row = (uint32_t)hd[11], A.bw = bw, A.bh = bh;
    A.write_back = 1;
    for (uint32_t t = 0; t < n_tiles; t++) md_ifs_emit_trial(A, t / trials, t, md_ifs_trial(walk, t % trials));
    for (uint32_t i = 0; i < n_cand; i++) refused += md_ifs_walk(A, i, walk);

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    wr(fo, result), wr(fo, std::vector<int32_t>{(int32_t)refused_tiles});
    fwrite(t_pu, sizeof(svthip_inter_pu_desc), n_tiles, fo);
    wr(fo, t_desc), wr(fo, found);
    fwrite(pu, sizeof(svthip_inter_pu_desc), n_cand, fo);
    wr(fo, std::vector<int32_t>{(int32_t)refused});
    fclose(fo);
    free(pu);
    free(t_pu);
    return 0;
}
