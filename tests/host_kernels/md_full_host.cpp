// tests/host_kernels/md_full_host.cpp -- the __device__ arithmetic and index geometry of svt-av1-1_amd/csrc/md_full_kernels.h compiled by g++ behind
// hip_on_host.h: the expansion of the picks into slot states and TU / rate / search descriptors (md_full_expand_luma, _chroma), the take-over
// of a search's winner (md_full_luma_winner), the cost of a slot (md_full_cost), the decision of a group (md_full_decide) and the copy of the
// winner's tile (md_full_copy_quad).  What the chain and the rate kernels leave in the workspace -- eobs, sums, bits, the DC level, the
// winner of the search -- comes from the caller (the restatement's numbers), as do the slot planes after the chain.  The slot planes and the
// reconstructed picture are allocated to exactly their size, `shift` bytes into their allocations, so under -fsanitize=address a copy that
// leaves a tile or a block ends the run.  The chain, the rate and the vector stores are the GPU test's business.
//   usage: md_full_host IN OUT
//   IN:  int32 head[24]: bw, bh, n_cand, n_groups, max_full, tiles_per_row, mask_inter, mask_intra, reduced, shift, src strides (Y, C), pool
//        strides (Y, C), slot plane w, h, cw, ch, recon plane w, h, cw, ch, n_types, tx_size_y; uint8 types[16]; uint32 iscan_y[16], iscan_uv[16];
//        svthip_md_fast_desc[n_cand]; svthip_md_full_desc[n_cand]; svthip_md_fast_group[n_groups]; svthip_md_fast_pick[n_groups]; per slot
//        (n = n_groups * max_full): uint16 eob[3][n], uint64 energy[n], uint64 dist[3][n][2], uint32 bits[3][n], int32 dc[3][n], uint8 winner
//        type index[n]; the slot planes Y, Cb, Cr; the reconstructed picture Y, Cb, Cr
//   OUT: MdFullSlot[n], svthip_tu_desc[3][n], svthip_coeff_rate_desc[3][n], svthip_tu_desc[m], svthip_coeff_rate_desc[m] (m = n * n_types),
//        tx_search_tu_dev[n], uint32 bases[304], svthip_md_full_result[n], svthip_md_full_decision[n_groups], the reconstructed picture,
//        int32 refused
#include "hip_on_host.h"

#include <memory>

#include "md_full_kernels.h"

using namespace svthip;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    const std::vector<int32_t> hd = rd<int32_t>(fi, 24);
    const std::vector<uint8_t> types = rd<uint8_t>(fi, 16);
    const std::vector<uint32_t> iscan_y = rd<uint32_t>(fi, 16), iscan_uv = rd<uint32_t>(fi, 16);
    MdFullArgs A;
    memset(&A, 0, sizeof(A));
    A.bw = (uint32_t)hd[0], A.bh = (uint32_t)hd[1], A.n_cand = (uint32_t)hd[2], A.n_groups = (uint32_t)hd[3], A.max_full = (uint32_t)hd[4];
    A.tiles_per_row = (uint32_t)hd[5], A.mask_inter = (uint32_t)hd[6], A.mask_intra = (uint32_t)hd[7], A.reduced_tx_set = (uint8_t)hd[8];
    const size_t shift = (size_t)hd[9];
    A.src_stride[0] = (uint32_t)hd[10], A.src_stride[1] = (uint32_t)hd[11], A.pred_stride[0] = (uint32_t)hd[12], A.pred_stride[1] = (uint32_t)hd[13];
    A.slot_stride[0] = (uint32_t)hd[14], A.slot_stride[1] = (uint32_t)hd[16], A.recon_stride[0] = (uint32_t)hd[18], A.recon_stride[1] = (uint32_t)hd[20];
    A.n_types = (uint32_t)hd[22], A.tx_size_y = hd[23];
    if (A.tx_size_y != md_full_tx_size(A.bw, A.bh)) return 3;
    A.n_slots = A.n_groups * A.max_full;
    A.cw = A.bw / 2u < 4u ? 4u : A.bw / 2u, A.ch = A.bh / 2u < 4u ? 4u : A.bh / 2u;
    A.tile_w = A.bw < 8u ? 8u : A.bw, A.tile_h = A.bh < 8u ? 8u : A.bh;
    A.ncoef[0] = (A.bw < 32u ? A.bw : 32u) * (A.bh < 32u ? A.bh : 32u), A.ncoef[1] = A.cw * A.ch;
    A.shift_y = md_full_dist_shift(A.bw, A.bh), A.shift_uv = md_full_dist_shift(A.cw, A.ch);
    for (int t = 0; t < 16; t++) A.types[t] = types[t], A.iscan_y[t] = iscan_y[t], A.iscan_uv[t] = iscan_uv[t];
    const uint32_t n = A.n_slots, m = n * A.n_types;

    const std::vector<svthip_md_fast_desc> fast = rd<svthip_md_fast_desc>(fi, A.n_cand);
    const std::vector<svthip_md_full_desc> full = rd<svthip_md_full_desc>(fi, A.n_cand);
    const std::vector<svthip_md_fast_group> group = rd<svthip_md_fast_group>(fi, A.n_groups);
    const std::vector<svthip_md_fast_pick> pick = rd<svthip_md_fast_pick>(fi, A.n_groups);
    std::vector<uint16_t> eob = rd<uint16_t>(fi, 3u * n);
    std::vector<uint64_t> energy = rd<uint64_t>(fi, n), dist = rd<uint64_t>(fi, 6u * n);
    std::vector<uint32_t> bits = rd<uint32_t>(fi, 3u * n);
    const std::vector<int32_t> dc = rd<int32_t>(fi, 3u * n);
    const std::vector<uint8_t> winner = rd<uint8_t>(fi, n);
    const size_t dims[6][2] = {{(size_t)hd[14], (size_t)hd[15]}, {(size_t)hd[16], (size_t)hd[17]}, {(size_t)hd[16], (size_t)hd[17]},
                               {(size_t)hd[18], (size_t)hd[19]}, {(size_t)hd[20], (size_t)hd[21]}, {(size_t)hd[20], (size_t)hd[21]}};
    std::unique_ptr<uint8_t[]> mem[6];   // new[] of exactly shift + width * height bytes: a vector may keep capacity behind its size
    for (int p = 0; p < 6; p++) {
        const std::vector<uint8_t> plane = rd<uint8_t>(fi, dims[p][0] * dims[p][1]);
        mem[p].reset(new uint8_t[shift + plane.size()]);
        memset(mem[p].get(), 0x5A, shift);
        memcpy(mem[p].get() + shift, plane.data(), plane.size());
    }
    fclose(fi);
    A.fast = fast.data(), A.full = full.data(), A.group = group.data(), A.pick = pick.data();
    for (int p = 0; p < 3; p++) A.slot_plane[p] = mem[p].get() + shift, A.recon_plane[p] = mem[3 + p].get() + shift;

    std::vector<MdFullSlot> slots(n);
    std::vector<svthip_tu_desc> tu(3u * n), s_tu(m);
    std::vector<svthip_coeff_rate_desc> rate(3u * n), s_rate(m);
    std::vector<tx_search_tu_dev> s_tus(n);
    std::vector<uint32_t> bases(19 * 16, 0xdeadbeefu), s_bits(m, 0x7777u);
    std::vector<uint64_t> s_energy(m, 0x1234u), s_dist(2u * m, 0x4321u);
    std::vector<svthip_tx_search_result> s_out(n);
    std::vector<int32_t> qcoeff[3];
    std::vector<svthip_md_full_result> result(n);
    std::vector<svthip_md_full_decision> decision(A.n_groups);
    uint32_t refused = 0;
    A.slots = slots.data(), A.energy_y = energy.data();
    for (int p = 0; p < 3; p++) {
        A.tu[p] = tu.data() + (size_t)p * n, A.rate[p] = rate.data() + (size_t)p * n;
        A.eob[p] = eob.data() + (size_t)p * n, A.dist[p] = dist.data() + (size_t)p * 2u * n, A.bits[p] = bits.data() + (size_t)p * n;
        qcoeff[p].assign((size_t)n * A.ncoef[p ? 1 : 0], 0x0badf00d);
        for (uint32_t k = 0; k < n; k++) qcoeff[p][(size_t)k * A.ncoef[p ? 1 : 0]] = dc[(size_t)p * n + k];
        A.qcoeff[p] = qcoeff[p].data();
    }
    A.s_tu = s_tu.data(), A.s_rate = s_rate.data(), A.s_tus = s_tus.data(), A.s_bases = bases.data();
    A.s_energy = s_energy.data(), A.s_dist = s_dist.data(), A.s_bits = s_bits.data(), A.s_out = s_out.data();
    A.result = result.data(), A.decision = decision.data(), A.refused = &refused;

    for (uint32_t k = 0; k < n; k++) refused += md_full_expand_luma(A, k);
    if (A.n_types) {
        // what the chain, the rate and the decision leave for the winner: the slot's numbers at the winner's candidate, nothing of them in the slot
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t pos = winner[k] * n + k;
            s_dist[2u * pos] = dist[2u * k], s_dist[2u * pos + 1u] = dist[2u * k + 1u], s_energy[pos] = energy[k], s_bits[pos] = bits[k];
            dist[2u * k] = dist[2u * k + 1u] = energy[k] = 0x5555u, bits[k] = 0x5555u;
            memset(&s_out[k], 0, sizeof(s_out[k]));
            s_out[k].candidate = pos, s_out[k].tx_type = A.types[winner[k]];
        }
        for (uint32_t k = 0; k < n; k++) md_full_luma_winner(A, k);
    }
    for (uint32_t k = 0; k < n; k++) md_full_expand_chroma(A, k);
    for (uint32_t k = 0; k < n; k++) result[k] = md_full_cost(A, k);
    for (uint32_t g = 0; g < A.n_groups; g++) decision[g] = md_full_decide(A, g);
    const uint32_t quads = md_full_copy_quads(A.bw, A.bh, A.cw, A.ch);
    for (uint32_t g = 0; g < A.n_groups; g++)
        for (uint32_t q = 0; q < quads; q++) md_full_copy_quad(A, g, q);

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    wr(fo, slots), wr(fo, tu), wr(fo, rate);
    if (m) wr(fo, s_tu), wr(fo, s_rate);   // empty without a search: fwrite takes no null pointer
    wr(fo, s_tus), wr(fo, bases), wr(fo, result), wr(fo, decision);
    for (int p = 3; p < 6; p++) fwrite(mem[p].get() + shift, 1, dims[p][0] * dims[p][1], fo);
    wr(fo, std::vector<int32_t>{(int32_t)refused});
    fclose(fo);
    return 0;
}
