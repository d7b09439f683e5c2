// svt-av1-1_amd/csrc/me_kernels.h -- internal declarations shared by the HIP kernels and the C-ABI glue.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svtav1_hip.h"
#include "tq_tile.h"
#include "tq_tx_search_tu.h"

// LDS row pitch of the staged reference window.  192 B: >= 16*8 + 64 (widest lane footprint at
// search_area_width 127) and == 48 dwords, which puts rows y, y+3, y+5, y+6 (one ds_read_b128 lane
// group) on four distinct bank quarters.
#define SVTHIP_FULLPEL_LDS_PITCH 192
// fixed LDS in front of the window: 16 KB exchange buffer + 64 B
#define SVTHIP_FULLPEL_LDS_FIXED (16384 + 64)

namespace svthip {

// XCD-aware block -> work-item map for the per-superblock kernels.  The dispatcher deals consecutive workgroups round-robin over the 8
// XCDs (MI355X_MICROARCH.md: blocks b and b + 8 share an XCD), and every XCD has its own 4 MB L2: with item = blockIdx, raster
// neighbours -- whose search windows overlap by half -- land on 8 different L2s and each fetches the overlap for itself.  With
//     item = (b % 8) * ceil(n / 8) + b / 8          (grid = 8 * ceil(n / 8) blocks, items >= n exit at once)
// an XCD works through one contiguous eighth of the superblock list, so the overlapping window rows are L2 hits.  Placement is used
// for speed only: any block -> XCD assignment gives the same results.
__host__ __device__ inline uint32_t xcd_grid(uint32_t n) { return 8u * ((n + 7u) >> 3); }
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t xcd_item(uint32_t b, uint32_t n) { return (b & 7u) * ((n + 7u) >> 3) + (b >> 3); }
#endif

__global__ void fullpel85_kernel(const uint8_t* __restrict__ src_plane, uint32_t src_stride,
                                 const uint8_t* __restrict__ ref_plane, uint32_t ref_stride,
                                 const int32_t* __restrict__ desc, uint32_t n_sb, uint32_t* __restrict__ out_sad,
                                 uint32_t* __restrict__ out_mv);

// job table of one search-centre launch, passed by value in the kernel arguments (2.5 KB)
struct HmeJobTable {
    svthip_pa_picture cur[SVTHIP_HME_MAX_JOBS];
    svthip_pa_picture ref[SVTHIP_HME_MAX_JOBS];
};
__global__ void hme_center_kernel(const uint8_t* __restrict__ pool, HmeJobTable jobs, svthip_me_params P, uint32_t list_index,
                                  const svthip_sb_origin* __restrict__ sbs, uint32_t n_sb, uint32_t n_jobs, const uint32_t* __restrict__ l0_best_mv64,
                                  uint32_t l0_mv_stride, svthip_fullpel_desc* __restrict__ out_desc,
                                  int16_t* __restrict__ out_center, int16_t* __restrict__ hme_state);

// job table of one picture-analysis launch (pa_planes.hip), passed by value
struct PaJobTable {
    svthip_pa_picture pic[SVTHIP_HME_MAX_JOBS];
};
__global__ void pa_derive_planes_kernel(uint8_t* __restrict__ pool, PaJobTable jobs, int do_quarter, int do_sixteenth);
__global__ void me_results_ref_layout_kernel(const svthip_me_cu_result* __restrict__ in, uint32_t n, svthip_me_cu_result_ref* __restrict__ out);
__global__ void ois_kernel(const uint8_t* __restrict__ pool, PaJobTable jobs, svthip_ois_params P, const svthip_sb_origin* __restrict__ sbs,
                           uint32_t n_sb, uint32_t n_jobs, const svthip_me_cu_result* __restrict__ me, uint32_t me_stride,
                           uint32_t* __restrict__ out_cand, uint8_t* __restrict__ out_total);
hipError_t launch_pad_plane(void* plane, uint32_t stride, int width, int height, int pad_w, int pad_h, int sample_bytes, hipStream_t s);

__global__ void subpel_planes_kernel(const uint8_t* __restrict__ src_plane, uint32_t src_stride, const uint8_t* __restrict__ ref_plane,
                                     uint32_t ref_stride, const int32_t* __restrict__ desc, uint32_t n_sb, int disable_8x8, int n_pu,
                                     uint32_t* __restrict__ io_sad, uint32_t* __restrict__ io_mv, uint32_t* __restrict__ pred_out, int method);
size_t subpel_planes_lds_bytes(uint32_t max_sw, uint32_t max_sh);
uint32_t subpel_planes_grid(uint32_t n_sb);
__global__ void bipred_stored_pack_kernel(const uint8_t* __restrict__ src_plane, uint32_t src_stride, const int32_t* __restrict__ desc0,
                                          const uint8_t* __restrict__ pred0, const uint8_t* __restrict__ pred1,
                                          const uint32_t* __restrict__ sad0, const uint32_t* __restrict__ mv0,
                                          const uint32_t* __restrict__ sad1, const uint32_t* __restrict__ mv1, int n_pu, int bipred_8x8,
                                          svthip_me_cu_result* __restrict__ out);
__global__ void bipred_nsq_pack_kernel(const uint8_t* __restrict__ src_plane, uint32_t src_stride,
                                       const uint8_t* __restrict__ ref0_plane, uint32_t ref0_stride, const int32_t* __restrict__ desc0,
                                       const uint8_t* __restrict__ ref1_plane, uint32_t ref1_stride, const int32_t* __restrict__ desc1,
                                       const uint32_t* __restrict__ sad0, const uint32_t* __restrict__ mv0,
                                       const uint32_t* __restrict__ sad1, const uint32_t* __restrict__ mv1, int n_lists, int win_bytes,
                                       const uint32_t* __restrict__ bisad_sq, svthip_me_cu_result* __restrict__ out);
size_t bipred_nsq_lds_bytes(uint32_t max_sw, uint32_t max_sh);
__global__ void bipred_pack_kernel(const uint8_t* __restrict__ src_plane, uint32_t src_stride,
                                   const uint8_t* __restrict__ ref0_plane, uint32_t ref0_stride, const int32_t* __restrict__ desc0,
                                   const uint8_t* __restrict__ ref1_plane, uint32_t ref1_stride, const int32_t* __restrict__ desc1,
                                   const uint32_t* __restrict__ sad0, const uint32_t* __restrict__ mv0,
                                   const uint32_t* __restrict__ sad1, const uint32_t* __restrict__ mv1, int n_lists, int bipred_8x8,
                                   int win_bytes, int pu_stride, uint32_t* __restrict__ bisad_out,
                                   svthip_me_cu_result* __restrict__ out);
size_t subpel_window_bytes(uint32_t max_sw, uint32_t max_sh);
size_t bipred_lds_bytes(uint32_t max_sw, uint32_t max_sh);

__global__ void quantize_b_batch_kernel(const int32_t* __restrict__ coeff, const svthip_quant_desc* __restrict__ desc, uint32_t n_tu,
                                        const int16_t* __restrict__ qparams, const int16_t* __restrict__ iscan_pool,
                                        int32_t* __restrict__ qcoeff, int32_t* __restrict__ dqcoeff, uint16_t* __restrict__ eob);

bool fwd_txfm2d_size_valid(int w, int h);
bool fwd_txfm2d_type_valid(int w, int h, int tx_type);
hipError_t launch_fwd_txfm2d(const int16_t* residual, const svthip_txfm_desc* desc, uint32_t n_tu, int w, int h, int32_t* coeff,
                             hipStream_t s);

hipError_t launch_inv_txfm2d_add(const int32_t* coeff, const svthip_itxfm_desc* desc, uint32_t n_tu, int w, int h, int bd,
                                 void* recon, int recon_16bit, hipStream_t s);

hipError_t launch_encode_tu(const void* src, const void* pred, void* recon, int planes_16bit, const svthip_tu_desc* desc, uint32_t n_tu,
                            int w, int h, const int16_t* qparams, const int16_t* iscan, int32_t* coeff, int32_t* qcoeff,
                            int32_t* dqcoeff, uint16_t* eob, uint64_t* energy, uint64_t* dist, uint32_t max_workgroups, hipStream_t s);
// the instantiations of the three transform kernels whose dynamic LDS passes 64 KB (svthip_abi.hip raises their limit once per device):
// one per size, x 2 sample types (inverse, fused), x 2 with / without distortion sums (fused)
constexpr int kFwdTxfmDynamicLdsKernels = tx_dynamic_lds_sizes(false), kInvTxfmDynamicLdsKernels = 2 * tx_dynamic_lds_sizes(false),
              kEncodeTuDynamicLdsKernels = 4 * tx_dynamic_lds_sizes(true);
#define SVTHIP_LOCAL __attribute__((visibility("hidden")))  // the library's exported symbol list stays as it is
SVTHIP_LOCAL void fwd_txfm_dynamic_lds_kernels(const void** list);
SVTHIP_LOCAL void inv_txfm_dynamic_lds_kernels(const void** list);
SVTHIP_LOCAL void encode_tu_dynamic_lds_kernels(const void** list);

// TxSize -> width / height (TX_4X4 .. TX_64X16, Codec/EbDefinitions.h)
__host__ __device__ inline int tx_w(int tx_size)
{
    constexpr uint8_t w[19] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64};
    return w[tx_size];
}
__host__ __device__ inline int tx_h(int tx_size)
{
    constexpr uint8_t h[19] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16};
    return h[tx_size];
}

// tq_coeff_rate.hip: the rate kernel (svthip_coeff_rate_batch_dev) and the batcher's RD decision.  A search TU on the device:
// tx_search_tu_dev (tq_tx_search_tu.h).
hipError_t launch_coeff_rate(const svthip_coeff_rate_tables* tables, const int32_t* qcoeff, const uint16_t* eob, const int16_t* iscan,
                             const svthip_coeff_rate_desc* desc, uint32_t n_tu, int tx_size, uint32_t* bits, hipStream_t s);
hipError_t launch_tx_decision(const tx_search_tu_dev* tus, uint32_t n_tus, const uint32_t* bases, const uint16_t* eob, const uint64_t* energy,
                              const uint64_t* dist, const uint32_t* bits, svthip_tx_search_result* out, hipStream_t s);

__global__ void fullpel209_kernel(const uint8_t* __restrict__ src_plane, uint32_t src_stride, const uint8_t* __restrict__ ref_plane,
                                  uint32_t ref_stride, const int32_t* __restrict__ desc, uint32_t n_sb, uint32_t* __restrict__ out_sad,
                                  uint32_t* __restrict__ out_mv);
size_t fullpel209_lds_bytes(uint32_t max_sh);

__global__ void sad_loop_kernel(const uint8_t* __restrict__ src, uint32_t src_stride, const uint8_t* __restrict__ ref, uint32_t ref_stride,
                                uint32_t ref_stride_raw, const svthip_sad_loop_desc* __restrict__ desc, uint32_t n_blocks, int w, int h, int sw, int sh,
                                int slice_bytes, uint32_t* __restrict__ best_sad, int16_t* __restrict__ best_xy);
bool convolve_mfma_size_valid(int w, int h);
bool convolve_size_valid(int w, int h);
// One launch of the convolution kernels on blocks of one size (ip_convolve.hip: the 22 AV1 sizes, any bd; ip_convolve_mfma.hip: sides that
// are multiples of 32, bd 8).  desc: svthip_convolve_desc (src1 unused) or, with compound, svthip_convolve_compound_desc.  counted: the block
// count is in device memory, in the 16 bytes in front of desc, and n_blocks only sizes the grid.  bd above 8: 16-bit planes, units are samples.
struct ConvolveLaunch {
    const void* src0; uint32_t stride0;
    const void* src1; uint32_t stride1;
    void* dst; uint32_t dst_stride;
    const void* desc; uint32_t n_blocks;
    int w, h, bd;
    bool compound, counted;
};
hipError_t launch_convolve_valu(const ConvolveLaunch& L, hipStream_t s);
hipError_t launch_convolve_mfma(const ConvolveLaunch& L, hipStream_t s);
// the instantiations whose dynamic LDS can pass 64 KB (svthip_abi.hip raises their limit once per device)
constexpr int kConvolveDynamicLdsKernels = 8;
void convolve_dynamic_lds_kernels(const void** list);
size_t sad_loop_qsad_lds_bytes(int w, int h, int sw, int sh, int k);  // workgroup LDS of the packed-SAD kernel (its own plan: blocks per workgroup, pitch)
hipError_t launch_sad_loop_qsad(const uint8_t* src, uint32_t src_stride, const uint8_t* ref, uint32_t ref_stride, uint32_t ref_stride_raw,
                                const svthip_sad_loop_desc* desc, uint32_t n_blocks, int w, int h, int sw, int sh, uint32_t* best_sad,
                                int16_t* best_xy, hipStream_t s);
size_t sad_loop_slice_bytes(int w, int h, int sw, int sh, int k);
// ip_inter_pred.hip: the descriptor expansion and the 2-wide / 2-high chroma pieces
hipError_t launch_inter_pred(const svthip_inter_planes& ref0, const svthip_inter_planes& ref1, const svthip_inter_planes& dst,
                             const svthip_inter_pu_desc* desc, uint32_t n_pu, int bw, int bh, int bd, bool use_mfma, void* scratch,
                             uint32_t* refused, hipStream_t s, uint8_t* refused_rows = nullptr);   // refused_rows[i] = 1 for a refused PU i
size_t inter_pred_scratch_bytes(uint32_t n_pu);
bool inter_pred_has_pieces(int bw, int bh);
// ip_warp.hip: warped-motion prediction of whole PUs (the warp kernel; translational chroma through the counted convolution kernels)
hipError_t launch_warped_pred(const svthip_inter_planes& ref, const svthip_inter_planes& dst, int pic_w, int pic_h, const svthip_warp_pu_desc* desc,
                              uint32_t n_pu, int bw, int bh, int bd, void* scratch, uint32_t* refused, hipStream_t s);
size_t warp_scratch_bytes(uint32_t n_pu);
bool warp_size_valid(int bw, int bh);
// ip_intra.hip: AV1 intra prediction of transform blocks of one TxSize (edges built on the device, optional SAD at 8 bits)
hipError_t launch_intra_pred(const void* edge, void* dst, const svthip_intra_desc* desc, uint32_t n_blocks, int tx_size, int bd, const uint8_t* src,
                             uint32_t* sad, uint32_t* refused, hipStream_t s);
bool intra_tx_size_valid(uint32_t tx_size);

// ip_cfl.hip: chroma-from-luma prediction, its 2 x 33 candidate tiles per block, and cfl_rd_pick_alpha's walk over their costs
hipError_t launch_cfl_pred(const void* luma, const void* cb, const void* cr, void* cb_dst, void* cr_dst, const svthip_cfl_desc* desc,
                           uint32_t n_blocks, int luma_w, int luma_h, int bd, uint32_t* refused, hipStream_t s);
hipError_t launch_cfl_candidates(const uint8_t* luma, const uint8_t* cb_dc, const uint8_t* cr_dc, const svthip_cfl_desc* desc, uint32_t n_blocks,
                                 int luma_w, int luma_h, uint8_t* candidates, hipStream_t s);
hipError_t launch_cfl_decision(const uint64_t* distortion, const uint32_t* bits, uint32_t dist_shift, const int32_t* alpha_bits,
                               const svthip_cfl_decision_job* job, uint32_t n_blocks, svthip_cfl_decision* out, hipStream_t s);
bool cfl_luma_size_valid(uint32_t w, uint32_t h);

// lf_deblock.hip: the deblocking filter of a picture, the SSE of every candidate level, and search_filter_level's walk over them
hipError_t launch_lf_frame(const svthip_lf_picture& pic, const svthip_lf_mi* mi, uint32_t mi_stride, const int32_t* levels, int sharpness,
                           int plane_start, int plane_end, int bd, hipStream_t s);
hipError_t launch_lf_sse_table(const svthip_lf_picture& pic, const svthip_lf_mi* mi, uint32_t mi_stride, int plane, int dir,
                               const int32_t* levels, int sharpness, int bd, uint64_t* sse, hipStream_t s);
hipError_t launch_lf_walk(const uint64_t* sse, int start_level, int only_4x4, int32_t* out0, int32_t* out1, uint64_t* visited, hipStream_t s);
hipError_t launch_lf_set_levels(int32_t* levels, const int32_t v[4], hipStream_t s);

// lr_wiener.hip: Wiener loop restoration -- the unit geometry, the statistics, the solve, the unit filter as SSE trial, the refinement walk
// step by step and as the whole search, and the frame filter of the three unit types (kernels: lr_wiener_kernels.h)
struct LrWorkspace {   // byte offsets into the caller's workspace, and its size
    size_t raw, M, H, sse_none, trial_sse, state, start_taps, avg, rejected, total;
};
LrWorkspace lr_workspace(uint32_t n_units);
uint32_t lr_unit_geometry(uint32_t width, uint32_t height, const uint32_t unit_size[3], uint32_t unit_base[4], int32_t* limits);
uint32_t lr_walk_max_trials(int win);
hipError_t launch_lr_stats(const svthip_lr_picture& pic, int plane_start, int plane_end, int bd, void* raw, int64_t* M, int64_t* H, int32_t* avg,
                           int64_t* sse_none, hipStream_t s);
hipError_t launch_lr_solve(const int64_t* M, const int64_t* H, uint32_t unit_begin, uint32_t unit_end, int win, int16_t* taps, int32_t* rejected,
                           hipStream_t s);
hipError_t launch_lr_trial(const svthip_lr_picture& pic, int plane_start, int plane_end, int bd, const void* taps, size_t taps_stride,
                           const uint8_t* skip, size_t skip_stride, int64_t* sse, hipStream_t s);
hipError_t launch_lr_filter_frame(const svthip_lr_picture& pic, void* const out[3], const uint32_t out_stride[3], int plane_start, int plane_end,
                                  int bd, const uint8_t* unit_type, const int16_t* taps, const int32_t* sgrproj, uint32_t* refused, hipStream_t s);
hipError_t launch_lr_walk_init(svthip_wiener_walk_state* state, const int16_t* taps, const int32_t* rejected, uint32_t unit_begin, uint32_t unit_end,
                               int win, hipStream_t s);
hipError_t launch_lr_walk_step(svthip_wiener_walk_state* state, const int64_t* trial_sse, uint32_t unit_begin, uint32_t unit_end, int32_t* pending,
                               hipStream_t s);
SVTHIP_LOCAL hipError_t launch_lr_search(const svthip_lr_picture& pic, int plane_start, int plane_end, int bd, uint32_t n_steps, bool resume,
                                         void* work, int64_t* sse, int16_t* taps, int32_t* n_trials, int32_t* pending, hipStream_t s);
// lr_sgrproj.hip: self-guided loop restoration -- the box filter over a plane, the solve, the walk on tables, the whole search, the unit
// filter as SSE trial and as the self-guided pass of launch_lr_filter_frame (kernels: lr_sgrproj_kernels.h)
struct SgrWorkspace {   // byte offsets into the caller's workspace, and its size
    size_t sums, err, size, ep, ntr, xq, start, fin, f[3], total;
};
SgrWorkspace sgr_workspace(uint32_t width, uint32_t height);
uint32_t sgr_walk_max_trials();
hipError_t launch_sgr_plane(const svthip_lr_picture& pic, int plane, int bd, int ep, int32_t* flt0, int32_t* flt1, uint32_t flt_stride, hipStream_t s);
hipError_t launch_sgr_solve(const int64_t* sums, const int32_t* size, const int32_t* ep, uint32_t n, int32_t* xq, int32_t* xqd, hipStream_t s);
hipError_t launch_sgr_walk_table(const int64_t* tables, const int32_t* ep, const int32_t* start, uint32_t n, int32_t* xqd, int64_t* err, int32_t* n_trials,
                                 hipStream_t s);
hipError_t launch_sgr_search(const svthip_lr_picture& pic, int plane_start, int plane_end, int bd, void* work, int32_t* sgrproj, int64_t* sse,
                             svthip_sgrproj_detail* detail, hipStream_t s);
hipError_t launch_sgr_trial(const svthip_lr_picture& pic, int plane_start, int plane_end, int bd, const int32_t* sgrproj, const uint8_t* skip, int64_t* sse,
                            hipStream_t s);
SVTHIP_LOCAL hipError_t launch_sgr_filter_frame(const svthip_lr_picture& pic, void* const out[3], const uint32_t out_stride[3], int plane_start,
                                                int plane_end, int bd, const uint8_t* unit_type, const int32_t* sgrproj, uint32_t* refused,
                                                hipStream_t s);
// cf_cdef.hip: CDEF -- the strength search over all filter blocks, the strength pick, the frame filter, dist_8x8 on block pairs
// (kernels: cf_cdef_kernels.h)
double cdef_lambda(int base_qindex, int bd);
hipError_t launch_cdef_search_mse(const svthip_cdef_picture& pic, int base_qindex, int bd, uint64_t* mse, uint8_t* counted, hipStream_t s);
hipError_t launch_cdef_pick(const uint64_t* mse, const uint8_t* counted, uint32_t nfb, int base_qindex, int bd, svthip_cdef_result* result,
                            int8_t* fb_strength, hipStream_t s);
hipError_t launch_cdef_frame(const svthip_cdef_picture& pic, const svthip_cdef_result* result, const int8_t* fb_strength, int plane_start,
                             int plane_end, int bd, hipStream_t s);
hipError_t launch_cdef_dist_8x8(const uint16_t* dst, const uint16_t* src, uint32_t n, int coeff_shift, uint64_t* out, hipStream_t s);
// pa_stats.hip: picture-analysis statistics -- block means / variances, homogeneity, histograms (kernels: pa_stats_kernels.h)
hipError_t launch_pa_block_stats(const uint8_t* pool, const svthip_pa_picture* pics, const int64_t* chroma_offsets, uint32_t n, uint32_t chroma_stride,
                                 int sub_precision, uint32_t n_sb, uint8_t* y_mean, uint16_t* variance, uint8_t* cb_mean, uint8_t* cr_mean, hipStream_t s);
hipError_t launch_pa_homogeneity(const uint16_t* variance, uint32_t width, uint32_t height, uint32_t n, uint32_t n_sb, uint64_t* var_of_var32x32,
                                 uint8_t* homogeneous, uint32_t* picture, hipStream_t s);
inline size_t pa_region_sum_bytes(size_t n) { return sizeof(uint32_t) * 16 * 3 * n; }  // SLOT_PA_REGION_SUMS: [n][16][3]
hipError_t launch_pa_histograms(const uint8_t* pool, const svthip_pa_picture* pics, const int64_t* chroma_offsets, uint32_t n, uint32_t chroma_stride,
                                uint32_t* histogram, uint32_t* region_intensity, uint32_t* average_intensity, uint32_t* region_sum, hipStream_t s);
// pa_noise.hip: input-picture noise detection and the weak denoising arms (kernels: pa_noise_kernels.h)
hipError_t launch_pa_noise_detect(const uint8_t* pool, const svthip_pa_picture* pics, uint32_t n, int sub_precision, uint32_t n_sb, uint8_t* denoised,
                                  uint32_t denoised_stride, uint64_t* sb_var, uint8_t* flat_noise, uint32_t* picture, hipStream_t s);
hipError_t launch_pa_denoise(uint8_t* pool, const svthip_pa_picture* pics, const int64_t* chroma_offsets, uint32_t n, uint32_t chroma_stride, uint32_t n_sb,
                             uint8_t* denoised, uint32_t denoised_stride, const uint8_t* flat_noise, const uint32_t* picture, hipStream_t s);
// fg_grain.hip: AV1 film-grain synthesis -- the templates and scaling tables, the frame pass (kernels: fg_grain_kernels.h)
hipError_t launch_film_grain_tables(const svthip_film_grain_params& params, int bit_depth, int16_t* tables, hipStream_t s);
hipError_t launch_film_grain_frame(const svthip_film_grain_params& params, int bit_depth, const void* const src[3], const uint32_t src_stride[3],
                                   void* const dst[3], const uint32_t dst_stride[3], uint32_t width, uint32_t height, const int16_t* tables, hipStream_t s);
// md_fast.hip: mode decision's fast loop -- SADs and fast cost of predicted PUs, the pick for the full loop (kernels: md_fast_kernels.h)
hipError_t launch_md_fast_cost(const svthip_inter_planes& src, const svthip_inter_planes& pred, const svthip_md_fast_desc* desc, uint32_t n_cand,
                               uint32_t bwidth, uint32_t bheight, svthip_md_fast_result* result, hipStream_t s);
hipError_t launch_md_fast_pick(const svthip_md_fast_result* result, const svthip_md_fast_desc* desc, uint32_t n_cand, const svthip_md_fast_group* group,
                               uint32_t n_groups, svthip_md_fast_pick* pick, uint32_t* refused, hipStream_t s);
// md_ifs.hip: mode decision's interpolation-filter search -- SSE and modelled rate / distortion of predicted tiles, the search over the
// filter pairs through launch_inter_pred (kernels: md_ifs_kernels.h)
struct MdIfsLayout {
    size_t t_pu, t_desc, t_result, t_refused, unread_counter, y, cb, cr, total;   // byte offsets into the search's scratch, its size
    uint32_t tiles_per_row, y_stride, c_stride;                                  // the grid of trial tiles
};
bool md_ifs_size_ok(uint32_t bwidth, uint32_t bheight);
uint32_t md_ifs_trials(int32_t search_mode, int32_t enable_dual_filter);   // trial tiles per candidate: 9 full, 3 fast or without the dual filter
bool md_ifs_layout(uint64_t n_tiles, uint32_t bw, uint32_t bh, MdIfsLayout* L);   // false: more tiles than 16-bit positions address
hipError_t launch_md_model_rd(const svthip_inter_planes& src, const svthip_inter_planes& pred, const svthip_md_model_rd_desc* desc, uint32_t n_tiles,
                              uint32_t bwidth, uint32_t bheight, int16_t quantizer, svthip_md_model_rd_result* result, uint32_t* refused, hipStream_t s);
hipError_t launch_md_ifs_search(const svthip_inter_planes& ref0, const svthip_inter_planes& ref1, const svthip_inter_planes& src,
                                svthip_inter_pu_desc* pu, const svthip_md_ifs_desc* ifs, uint32_t n_cand, uint32_t bwidth, uint32_t bheight,
                                int32_t search_mode, int32_t enable_dual_filter, int16_t quantizer, int32_t write_back, svthip_md_ifs_result* result,
                                bool use_mfma, void* scratch, const MdIfsLayout& L, void* jobs_scratch, uint32_t* refused, hipStream_t s);
// md_full.hip: mode decision's full loop -- per slot the fused chain and the rate on Y, Cb and Cr with the tx-type search, the full cost,
// the decision per block, the winner's reconstruction (kernels: md_full_kernels.h)
struct MdFullLayout {   // byte offsets into the caller's workspace, its size, and the TxTypes a search runs
    size_t slots, tu[3], rate[3], eob[3], dist[3], bits[3], qcoeff[3], energy_y;
    size_t s_tu, s_rate, s_eob, s_energy, s_dist, s_bits, s_qcoeff, s_recon, s_tus, s_bases, s_out, total;
    uint32_t n_slots, n_types;   // n_types 0: no search
    uint8_t types[16];
};
struct MdFullCall {   // the arguments of svthip_md_full_loop_batch_dev
    svthip_inter_planes src, pred, slot_recon, recon;
    const svthip_md_fast_desc* fast;
    const svthip_md_full_desc* full;
    const svthip_md_fast_group* group;
    const svthip_md_fast_pick* pick;
    uint32_t n_cand, n_groups, bwidth, bheight, max_full, tiles_per_row, type_mask_inter, type_mask_intra, stages;
    int32_t reduced_tx_set;
    const int16_t *qparams, *iscan;
    const uint32_t* iscan_offsets;   // host, [19 * 16]
    const svthip_coeff_rate_tables* tables;
    void* work;
    svthip_md_full_result* result;
    svthip_md_full_decision* decision;
    uint32_t* refused;
    uint32_t max_workgroups;         // SVTHIP_OPT_TQ_MAX_WORKGROUPS
};
bool md_full_size_ok(uint32_t bwidth, uint32_t bheight);
bool md_full_layout(uint32_t n_groups, uint32_t max_full, uint32_t bw, uint32_t bh, uint32_t mask_inter, uint32_t mask_intra, MdFullLayout* L);
hipError_t launch_md_full_loop(const MdFullCall& C, const MdFullLayout& L, hipStream_t s);

inline size_t fullpel_lds_bytes(uint32_t max_sh) { return SVTHIP_FULLPEL_LDS_FIXED + (size_t)(max_sh + 63) * SVTHIP_FULLPEL_LDS_PITCH; }

}  // namespace svthip
