// tests/host_kernels/md_part_host.cpp -- the __device__ code of svt-av1-1_amd/csrc/md_part_kernels.h compiled by g++ behind hip_on_host.h:
// the geometry from the index, the whole decision of a superblock (md_part_decide_sb with ONE lane, so its barriers are no-ops and the
// lane does every stage in order) and the composition (md_part_compose_sb with the slices and the 256 lanes of the launch, one after the
// other: they do not depend on each other).  The pool and the destination planes are allocated to exactly stride x height bytes, `shift` bytes into
// their allocations, so under -fsanitize=address a read or a write past a plane ends the run.  The stride is the width (pad 0: the
// widths 136 and 68 then allow units of 8 and 4 bytes at most) or, with pad 1, the width rounded up to 16 plus 16 -- a multiple of 16
// whatever the width, as real pictures have, which with shift 0 takes every tile at a 16-aligned position in the 16-byte unit; the
// test fills the columns past the width with a guard and finds them unchanged.  shift 2 gives the 2-byte unit, shift 3 the byte.
// MD_PART_UNIT_HOOK tallies the unit of every tile copied, so the test can tell which arms of md_part_copy_tile ran.  What this cannot
// show -- the lanes of a workgroup together, the LDS, the barriers -- is what tests/test_md_part_gpu.py is for.
//   usage: md_part_host IN OUT
//   IN:  int32 sb_size, intra, n_sb, n_leaf, n_decision, shift, pool_w, pool_h, w, h, pad; int32 fac_bits[220]; svthip_md_partition_sb[n_sb];
//        svthip_md_partition_leaf[n_leaf]; svthip_md_full_decision[n_decision]; the pool Y, Cb, Cr; the destination Y, Cb, Cr
//   OUT: svthip_md_partition_block[n_blocks]; svthip_md_partition_result[n_sb * n_blocks]; svthip_md_partition_final[n_sb * max_final];
//        uint32 count[n_sb]; int32 refused; uint32 tiles copied in units of 1, 2, 4, 8, 16 bytes; the destination Y, Cb, Cr (stride x height)
#include "hip_on_host.h"

#include <memory>

static uint32_t unit_tiles[5];
#define MD_PART_UNIT_HOOK(unit) unit_tiles[(unit) == 16u ? 4 : (unit) == 8u ? 3 : (unit) == 4u ? 2 : (unit) == 2u ? 1 : 0]++

#include "md_part_kernels.h"

using namespace svthip;

template <uint32_t SB>
static void decide(const MdPartArgs& A)
{
    std::unique_ptr<MdPartShared<SB>> S(new MdPartShared<SB>);
    for (uint32_t sb = 0; sb < A.n_sb; sb++) md_part_decide_sb<SB>(A, sb, *S, 0, 1);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    const std::vector<int32_t> hd = rd<int32_t>(fi, 11);
    const uint32_t sb_size = (uint32_t)hd[0], n_sb = (uint32_t)hd[2], n_leaf = (uint32_t)hd[3], n_decision = (uint32_t)hd[4];
    const size_t shift = (size_t)hd[5];
    const uint32_t pool_w = (uint32_t)hd[6], pool_h = (uint32_t)hd[7], w = (uint32_t)hd[8], h = (uint32_t)hd[9];
    const std::vector<int32_t> fac = rd<int32_t>(fi, 220);
    const std::vector<svthip_md_partition_sb> sbs = rd<svthip_md_partition_sb>(fi, n_sb);
    const std::vector<svthip_md_partition_leaf> leaves = rd<svthip_md_partition_leaf>(fi, n_leaf);
    const std::vector<svthip_md_full_decision> decisions = rd<svthip_md_full_decision>(fi, n_decision);
    const size_t widths[6][2] = {{pool_w, pool_h}, {pool_w / 2, (pool_h + 1) / 2}, {pool_w / 2, (pool_h + 1) / 2}, {w, h}, {(w + 1) / 2, (h + 1) / 2}, {(w + 1) / 2, (h + 1) / 2}};
    size_t dims[6][2];   // stride, height
    for (int p = 0; p < 6; p++) dims[p][0] = hd[10] ? (widths[p][0] + 15) / 16 * 16 + 16 : widths[p][0], dims[p][1] = widths[p][1];
    std::unique_ptr<uint8_t[]> mem[6];   // new[] of exactly shift + width * height bytes: a vector may keep capacity behind its size
    for (int p = 0; p < 6; p++) {
        const std::vector<uint8_t> plane = rd<uint8_t>(fi, dims[p][0] * dims[p][1]);
        mem[p].reset(new uint8_t[shift + plane.size()]);
        memset(mem[p].get(), 0x5A, shift);
        memcpy(mem[p].get() + shift, plane.data(), plane.size());
    }
    fclose(fi);

    const uint32_t n_blocks = md_part_blocks(sb_size), max_final = md_part_max_final(sb_size);
    std::vector<svthip_md_partition_block> geom(n_blocks);
    for (uint32_t i = 0; i < n_blocks; i++) geom[i] = md_part_geom(sb_size, i);
    std::vector<svthip_md_partition_result> result((size_t)n_sb * n_blocks);
    std::vector<svthip_md_partition_final> final_((size_t)n_sb * max_final);
    std::vector<uint32_t> count(n_sb);
    uint32_t refused = 0;

    MdPartArgs A = {};
    A.sb = sbs.data(), A.leaf = leaves.data(), A.decision = decisions.data();
    A.n_sb = n_sb, A.n_leaf = n_leaf, A.n_decision = n_decision, A.intra = (uint32_t)hd[1];
    const int rows[4] = {0, 4, 8, 10};
    for (int r = 0; r < 4; r++) A.bits[r][0] = fac[rows[r] * 11], A.bits[r][1] = fac[rows[r] * 11 + 3];
    A.result = result.data(), A.final_ = final_.data(), A.final_count = count.data(), A.refused = &refused;
    if (sb_size == 128) decide<128>(A);
    else decide<64>(A);

    MdPartComposeArgs B = {};
    B.leaf = leaves.data(), B.final_ = final_.data(), B.final_count = count.data(), B.n_sb = n_sb, B.n_leaf = n_leaf, B.max_final = max_final;
    for (int p = 0; p < 3; p++) B.pool[p] = mem[p].get() + shift, B.dst[p] = mem[3 + p].get() + shift;
    B.pool_stride[0] = (uint32_t)dims[0][0], B.pool_stride[1] = (uint32_t)dims[1][0], B.dst_stride[0] = (uint32_t)dims[3][0], B.dst_stride[1] = (uint32_t)dims[4][0];
    B.pool_w = pool_w, B.pool_h = pool_h, B.w = w, B.h = h, B.refused = &refused;
    const uint32_t slices = md_part_compose_slices(n_sb);   // the grid of the launch
    launch(dim3(n_sb, slices), MD_PART_THREADS, [&] { md_part_compose_sb(B, blockIdx.x, blockIdx.y, slices, threadIdx.x, blockDim.x); });

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    wr(fo, geom), wr(fo, result), wr(fo, final_), wr(fo, count), wr(fo, std::vector<int32_t>{(int32_t)refused});
    wr(fo, std::vector<uint32_t>(unit_tiles, unit_tiles + 5));
    for (int p = 3; p < 6; p++) fwrite(mem[p].get() + shift, 1, dims[p][0] * dims[p][1], fo);
    fclose(fo);
    return 0;
}
