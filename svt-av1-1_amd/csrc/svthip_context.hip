// svt-av1-1_amd/csrc/svthip_context.hip -- the part of the C-ABI glue that every kernel family shares (svthip_glue.h): the error text,
// context and scratch, the validators more than one family uses, and the context entries of include/svtav1_hip.h.
//
// Host side of the drop-in boundary: context/stream ownership, argument validation.  There is deliberately no CPU fallback here: a
// missing device or a failed launch is an error.  The entries of a family are in its <family>_abi.hip.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <new>

#include "svthip_glue.h"
#include "fg_launch.h"
#include "ip_launch.h"
#include "md_launch.h"
#include "me_launch.h"
#include "pa_launch.h"
#include "tq_launch.h"

namespace {

// ---------------------------------------------------------------- errors, context, scratch

thread_local char g_err[512] = "";

// One-time, process-wide, per device: every kernel that takes dynamic LDS gets its limit raised to what the largest legal launch needs
// (160 KB minus the kernel's static LDS; each file does it for its own kernels, svthip_internal.h).  hipFuncSetAttribute is
// per-FUNCTION state, so it must not be cached per context: a second context with a smaller search area would lower the limit under a
// first one's launches (round-1 defect).
std::once_flag g_attr_once[16];
hipError_t g_attr_status[16];

void set_kernel_attrs(int device)
{
    hipError_t st = hipSuccess;
    for (hipError_t (*raise)() : {svthip::fullpel85_raise_dynamic_lds, svthip::fullpel209_raise_dynamic_lds, svthip::bipred_raise_dynamic_lds,
                                  svthip::subpel_planes_raise_dynamic_lds, svthip::convolve_raise_dynamic_lds, svthip::fwd_txfm_raise_dynamic_lds,
                                  svthip::inv_txfm_raise_dynamic_lds, svthip::encode_tu_raise_dynamic_lds}) {
        const hipError_t e = raise();
        if (e != hipSuccess) st = e;
    }
    g_attr_status[device] = st;
}

}  // namespace

__attribute__((format(printf, 2, 3))) int32_t fail(int32_t code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// entry prologue of every call: the context's device becomes current for the calling thread
int32_t enter(svthip_ctx* c)
{
    if (!c) return fail(SVTHIP_ERR_BAD_PARAMETER, "null context");
    HIP_TRY(hipSetDevice(c->device));
    return SVTHIP_OK;
}

// Context-owned scratch is about to be used by work enqueued on `s`: if the previous user was a different stream, order `s` behind it
// (a caller may hand any stream to a `_dev` entry; two in-flight calls of one context on two streams then serialise instead of racing).
int32_t scratch_on_stream(svthip_ctx* c, hipStream_t s)
{
    if (c->scratch_stream && c->scratch_stream != s) {
        HIP_TRY(hipEventRecord(c->scratch_event, c->scratch_stream));
        HIP_TRY(hipStreamWaitEvent(s, c->scratch_event, 0));
    }
    c->scratch_stream = s;
    return SVTHIP_OK;
}

// Growing a slot is stream-ordered: the old buffer is released with hipFreeAsync behind the last stream that used the context's scratch
// (every earlier user is ordered before that stream, see scratch_on_stream) and the new one comes from hipMallocAsync on the same
// stream, so one context's growth never synchronises the device under the other contexts' work (hipFree would: round-2 finding).
// svthip_reserve pre-sizes the slots so that steady-state calls never get here.
int32_t ensure_scratch(svthip_ctx* c, Slot slot, size_t bytes)
{
    if (c->scratch_bytes[slot] >= bytes) return SVTHIP_OK;
    hipStream_t os = c->scratch_stream ? c->scratch_stream : c->stream;
    if (c->scratch[slot] && hipFreeAsync(c->scratch[slot], os) != hipSuccess) {
        (void)hipGetLastError();
        HIP_TRY(hipFree(c->scratch[slot]));
    }
    c->scratch[slot] = nullptr;
    c->scratch_bytes[slot] = 0;
    size_t want = bytes + bytes / 4 + 4096;
    if (hipMallocAsync(&c->scratch[slot], want, os) != hipSuccess) {
        (void)hipGetLastError();
        c->scratch[slot] = nullptr;
        return fail(SVTHIP_ERR_INSUFFICIENT_RESOURCES, "hipMallocAsync of device scratch failed (slot %d)", (int)slot);
    }
    c->scratch_bytes[slot] = want;
    c->scratch_stream = os;
    if (slot == SLOT_SB_TABLE) {
        // a new SB-origin table holds no geometry, whoever grew it (svthip_reserve or ensure_sb_table), and starts as all (0,0)
        // origins: were it ever read before ensure_sb_table filled it, every SB would see the first one's samples -- wrong results,
        // but no read outside the picture pool
        c->sb_table_w = c->sb_table_h = 0;
        HIP_TRY(hipMemsetAsync(c->scratch[slot], 0, want, os));
    }
    return SVTHIP_OK;
}

// raster SB origins of a w x h picture in SLOT_SB_TABLE, rebuilt only when the geometry changes or the slot was reallocated
// (ensure_scratch clears the cached geometry then); the upload is from pageable memory, so it is followed by a stream synchronisation;
// steady-state calls skip both
int32_t ensure_sb_table(svthip_ctx* c, uint32_t w, uint32_t h, hipStream_t s)
{
    const uint32_t nx = (w + 63) / 64, ny = (h + 63) / 64, n_sb = nx * ny;
    TRY(ensure_scratch(c, SLOT_SB_TABLE, sb_table_bytes(n_sb)));
    if (c->sb_table_w == w && c->sb_table_h == h) return SVTHIP_OK;
    svthip_sb_origin* sbs = new (std::nothrow) svthip_sb_origin[n_sb];
    if (!sbs) return fail(SVTHIP_ERR_INSUFFICIENT_RESOURCES, "out of host memory");
    for (uint32_t y = 0; y < ny; y++)
        for (uint32_t x = 0; x < nx; x++) sbs[y * nx + x] = svthip_sb_origin{(uint16_t)(x * 64), (uint16_t)(y * 64)};
    hipError_t e = hipMemcpyAsync(c->scratch[SLOT_SB_TABLE], sbs, sb_table_bytes(n_sb), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    delete[] sbs;
    HIP_TRY(e);
    c->sb_table_w = w;
    c->sb_table_h = h;
    return SVTHIP_OK;
}

// ---------------------------------------------------------------- validators

int32_t check_non_null(std::initializer_list<const void*> ps)
{
    for (const void* p : ps)
        if (!p) return fail(SVTHIP_ERR_BAD_PARAMETER, "null pointer argument");
    return SVTHIP_OK;
}

int32_t check_desc_aligned(const void* d_desc)
{
    return aligned(d_desc, 16) ? SVTHIP_OK : fail(SVTHIP_ERR_BAD_PARAMETER, "descriptor array must be 16-byte aligned");
}

bool n_pu_valid(uint32_t n_pu) { return n_pu == 85 || n_pu == 209; }
int32_t check_n_pu(uint32_t n_pu) { return n_pu_valid(n_pu) ? SVTHIP_OK : fail(SVTHIP_ERR_BAD_PARAMETER, "n_pu must be 85 or 209 (got %d)", (int)n_pu); }
int32_t check_av1_block(uint32_t w, uint32_t h)
{
    return svthip::convolve_size_valid((int)w, (int)h) ? SVTHIP_OK
                                                       : fail(SVTHIP_ERR_BAD_PARAMETER, "not an AV1 block size (width %d)", (int)w);
}

int32_t check_tx_size(uint32_t w, uint32_t h)
{
    return svthip::fwd_txfm2d_size_valid((int)w, (int)h) ? SVTHIP_OK
                                                         : fail(SVTHIP_ERR_BAD_PARAMETER, "unsupported transform size (width %d)", (int)w);
}
int32_t check_bit_depth_8_10(uint32_t bd) { return bd == 8 || bd == 10 ? SVTHIP_OK : fail(SVTHIP_ERR_BAD_PARAMETER, "bit_depth must be 8 or 10 (got %d)", (int)bd); }
int32_t check_bit_depth_10(uint32_t bd) { return bd == 10 ? SVTHIP_OK : fail(SVTHIP_ERR_BAD_PARAMETER, "bit_depth must be 10 (got %d)", (int)bd); }

// the pools of the fused transform / quantisation chain: a lane moves 4 coefficients (16 B) and 4 inverse-scan entries (8 B) at once
int32_t check_tq_pools(const void* coeff, const void* qcoeff, const void* dqcoeff, const void* iscan)
{
    if (!aligned({coeff, qcoeff, dqcoeff}, 16)) return fail(SVTHIP_ERR_BAD_PARAMETER, "coefficient pools must be 16-byte aligned");
    if (!aligned(iscan, 8)) return fail(SVTHIP_ERR_BAD_PARAMETER, "iscan pool must be 8-byte aligned");
    return SVTHIP_OK;
}

// ---------------------------------------------------------------- the three post-reconstruction filters

int32_t check_filter_picture_size(uint32_t width, uint32_t height)
{
    if (width == 0 || height == 0 || (width | height) % 8 != 0 || width > 16384 || height > 16384)
        return fail(SVTHIP_ERR_BAD_PARAMETER, "picture size must be a multiple of 8 each way, at most 16384 (got %ux%u)", (unsigned)width,
                    (unsigned)height);
    return SVTHIP_OK;
}

int32_t check_filter_bit_depth(int bd)
{
    return bd == 8 || bd == 10 ? SVTHIP_OK : fail(SVTHIP_ERR_BAD_PARAMETER, "bit depth must be 8 or 10 (got %d)", bd);
}

int32_t check_filter_planes(uint32_t p, uint32_t pw, int bd, const FilterPlane* planes, int n)
{
    for (int i = 0; i < n; i++) TRY(check_non_null({planes[i].base}));
    for (int i = 0; i < n; i++)
        if (planes[i].stride < pw) return fail(SVTHIP_ERR_BAD_PARAMETER, "stride of plane %d is smaller than its width %u", (int)p, (unsigned)pw);
    for (int i = 0; i < n; i++)
        if (bd > 8 && !aligned(planes[i].base, 2)) return fail(SVTHIP_ERR_BAD_PARAMETER, "16-bit planes must be 2-byte aligned");
    return SVTHIP_OK;
}

// ---------------------------------------------------------------- prediction and mode decision

// The two whole-PU prediction families (translational, warped) share SLOT_INTER_JOBS (job list; for the warped entries that of the
// translational chroma).  pred_check_args: the checks both make first, once there is work.  pred_begin: the rest of both prologues --
// 16-bit plane alignment, the family's PU cap, the call's stream and the refusal counter (refused_counter), the job list sized by the
// family's function.
int32_t pred_check_args(InterPlanesList planes, const void* d_desc)
{
    for (const svthip_inter_planes* p : planes) TRY(check_non_null({p}));
    TRY(check_non_null({d_desc}));
    for (const svthip_inter_planes* p : planes)
        if (!p->y || !p->cb || !p->cr) return fail(SVTHIP_ERR_BAD_PARAMETER, "null plane pointer");
    return check_desc_aligned(d_desc);
}

// What every entry that can refuse work on the device does last before it launches: the call's stream (the caller's, or the context's
// own), the context's scratch ordered on it, and on it the refusal counter of SLOT_REFUSED, cleared on its first use.
// svthip_inter_pred_refused synchronises with the stream of the last such call.
int32_t refused_counter(svthip_ctx* ctx, void* stream, hipStream_t* out_s, uint32_t** out_refused)
{
    hipStream_t s = call_stream(ctx, stream);
    TRY(scratch_on_stream(ctx, s));
    const bool first = ctx->scratch[SLOT_REFUSED] == nullptr;
    TRY(ensure_scratch(ctx, SLOT_REFUSED, 256));
    if (first) HIP_TRY(hipMemsetAsync(ctx->scratch[SLOT_REFUSED], 0, 256, s));
    ctx->refused_stream = s;
    *out_s = s;
    *out_refused = slot_ptr<uint32_t>(ctx, SLOT_REFUSED);
    return SVTHIP_OK;
}

int32_t pred_begin(svthip_ctx* ctx, InterPlanesList planes, int bd, uint32_t n_pu, uint32_t n_pu_cap, size_t (*scratch_bytes)(uint32_t),
                   void* stream, hipStream_t* out_s, uint32_t** out_refused)
{
    if (bd > 8)
        for (const svthip_inter_planes* p : planes)
            if (!aligned({p->y, p->cb, p->cr}, 2)) return fail(SVTHIP_ERR_BAD_PARAMETER, "16-bit planes must be 2-byte aligned");
    if (n_pu > n_pu_cap) return fail(SVTHIP_ERR_BAD_PARAMETER, "too many PUs in one call (%d)", (int)n_pu);
    TRY(refused_counter(ctx, stream, out_s, out_refused));
    TRY(ensure_scratch(ctx, SLOT_INTER_JOBS, scratch_bytes(n_pu)));
    return SVTHIP_OK;
}

extern "C" {

// ---------------------------------------------------------------- context and scratch

const char* svthip_last_error(void) { return g_err; }

int32_t svthip_create(int32_t device, svthip_ctx** out_ctx)
{
    if (!out_ctx) return fail(SVTHIP_ERR_BAD_PARAMETER, "out_ctx is null");
    *out_ctx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(SVTHIP_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(SVTHIP_ERR_BAD_PARAMETER, "device index out of range (%d)", device);
    if (device >= 16) return fail(SVTHIP_ERR_BAD_PARAMETER, "device index above 15 is not supported (%d)", device);
    HIP_TRY(hipSetDevice(device));
    std::call_once(g_attr_once[device], set_kernel_attrs, device);
    if (g_attr_status[device] != hipSuccess)
        return fail(SVTHIP_ERR_DEVICE, "raising the kernels' dynamic LDS limit failed: %s", hipGetErrorString(g_attr_status[device]));
    svthip_ctx* c = new (std::nothrow) svthip_ctx();
    if (!c) return fail(SVTHIP_ERR_INSUFFICIENT_RESOURCES, "out of host memory");
    memset(c, 0, sizeof(*c));
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(SVTHIP_ERR_DEVICE, "hipStreamCreate failed");
    }
    if (hipEventCreateWithFlags(&c->scratch_event, hipEventDisableTiming) != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return fail(SVTHIP_ERR_DEVICE, "hipEventCreate failed");
    }
    *out_ctx = c;
    return SVTHIP_OK;
}

void svthip_destroy(svthip_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (void* p : ctx->scratch)
        if (p) (void)hipFree(p);
    (void)hipEventDestroy(ctx->scratch_event);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

void* svthip_stream(svthip_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int32_t svthip_synchronize(svthip_ctx* ctx)
{
    TRY(enter(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SVTHIP_OK;
}

int32_t svthip_set_option(svthip_ctx* ctx, int32_t option, int32_t value)
{
    if (!ctx) return fail(SVTHIP_ERR_BAD_PARAMETER, "null context");
    if (option < 0 || option >= SVTHIP_OPT_COUNT) return fail(SVTHIP_ERR_BAD_PARAMETER, "unknown option %d", (int)option);
    ctx->opt[option] = value;
    return SVTHIP_OK;
}

int32_t svthip_reserve(svthip_ctx* ctx, uint32_t width, uint32_t height, uint32_t n_pu, uint32_t n_jobs, int32_t host_forms)
{
    TRY(enter(ctx));
    if ((width & 7) || (height & 7) || !width || !height || width > 16384 || height > 16384)
        return fail(SVTHIP_ERR_BAD_PARAMETER, "picture dimensions must be non-zero multiples of 8 (width %d)", (int)width);
    if (n_jobs == 0) n_jobs = 1;
    const size_t n_sb = sb_count(width, height), n = n_sb * n_jobs;
    if (n_pu == SVTHIP_INLOOP_ME_PU_COUNT)   // the in-loop search: its descriptors are all the scratch it has
    {
        TRY(ensure_scratch(ctx, SLOT_INLOOP_DESC, inloop_desc_bytes(n)));
        return ensure_scratch(ctx, SLOT_INLOOP_PLANES, svthip::inloop_planes_bytes(n));
    }
    TRY(check_n_pu(n_pu));
    TRY(ensure_scratch(ctx, SLOT_ME_CHAIN, me_chain_layout(n, n_pu).total));
    TRY(ensure_scratch(ctx, SLOT_BIPRED_SQ, bipred_sq_bytes(n)));
    TRY(ensure_scratch(ctx, SLOT_ME_PRED, me_pred_bytes(n, n_pu)));
    TRY(ensure_scratch(ctx, SLOT_PA_REGION_SUMS, svthip::pa_region_sum_bytes(SVTHIP_HME_MAX_JOBS)));
    TRY(ensure_scratch(ctx, SLOT_FILM_GRAIN_TABLES, SVTHIP_FILM_GRAIN_TABLES_BYTES));
    TRY(ensure_scratch(ctx, SLOT_FG_NOISE_MODEL, svthip::fg_noise_model_layout(width, height).total));
    TRY(ensure_scratch(ctx, SLOT_FG_FLAT_TABLES, sizeof(double) * SVTHIP_FILM_GRAIN_FLAT_TABLES_DOUBLES));
    TRY(ensure_scratch(ctx, SLOT_FG_DENOISE, svthip::fg_denoise_layout(width, height).planes));   // the one-call form's float planes grow it on first use
    TRY(ensure_scratch(ctx, SLOT_PA_SSE_PARTIALS, svthip::pa_sse_partial_bytes(width, height, n_jobs < SVTHIP_HME_MAX_JOBS ? n_jobs : SVTHIP_HME_MAX_JOBS)));
    {   // the interpolation-filter search in its fast mode, one 8x8 candidate per 8x8 block of a picture
        const uint64_t n_cand = (uint64_t)(width / 8) * (height / 8);
        svthip::MdIfsLayout L;
        if (svthip::md_ifs_layout(3 * n_cand, 8, 8, &L)) {
            TRY(ensure_scratch(ctx, SLOT_MD_IFS, L.total));
            TRY(ensure_scratch(ctx, SLOT_INTER_JOBS, svthip::inter_pred_scratch_bytes((uint32_t)(3 * n_cand))));
        }
    }
    if (host_forms) {
        TRY(ensure_scratch(ctx, SLOT_HOST_POOL, host_pool_layout(width, height).total(3)));
        TRY(ensure_scratch(ctx, SLOT_SB_TABLE, sb_table_bytes(n_sb)));
        TRY(ensure_scratch(ctx, SLOT_ME_RESULTS, me_results_bytes(n_sb, n_pu)));
        TRY(ensure_scratch(ctx, SLOT_ME_RESULTS_REF, me_results_ref_bytes(n_sb, n_pu)));
    }
    return SVTHIP_OK;
}

int32_t svthip_inter_pred_refused(svthip_ctx* ctx, uint32_t* out_count)
{
    TRY(enter(ctx));
    TRY(check_non_null({out_count}));
    *out_count = 0;
    uint32_t* d_refused = slot_ptr<uint32_t>(ctx, SLOT_REFUSED);
    if (!d_refused) return SVTHIP_OK;
    hipStream_t s = ctx->refused_stream ? ctx->refused_stream : ctx->stream;
    uint32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, d_refused, sizeof(n), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!n) return SVTHIP_OK;
    HIP_TRY(hipMemsetAsync(d_refused, 0, sizeof(n), s));
    *out_count = n;
    return fail(SVTHIP_ERR_BAD_PARAMETER, "%d PU(s) or unit(s) refused: BI_PRED with sub-8x8 chroma, a block outside the border its edges describe, an invalid warp model, an intra descriptor the reference would assert on, a CfL descriptor with alpha_signs > 7, a fast-loop group out of range (svthip_md_fast_pick_batch_dev), a tile at an odd position (svthip_md_model_rd_batch_dev), a candidate whose source position is odd or whose PU the prediction refuses (svthip_md_interp_filter_search_batch_dev), a pick or TxType (svthip_md_full_loop_batch_dev), or a restoration unit that is neither RESTORE_NONE nor RESTORE_WIENER (svthip_av1_[highbd_]lr_filter_frame_dev: a unit of an unknown type, one whose taps or self-guided parameters the call was not given, or self-guided parameters out of range)", (int)n);
}

}  // extern "C"
