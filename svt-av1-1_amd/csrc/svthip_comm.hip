// svt-av1-1_amd/csrc/svthip_comm.hip -- multi-GPU exchange behind the C ABI (include/svtav1_hip.h "Multi-GPU"), on RCCL directly.
//
// One rank per GPU (a process, or a thread of the reference's one process): every rank holds the read-only source planes, searches
// its share of the superblocks (no data-path collective), and reconstructs its SB-row slab of the picture.  What IS exchanged is the
// reconstructed reference picture -- the next picture's inter prediction reads all of it -- and, when a consumer wants them on every
// rank, the ME results.  Both are "every rank contributes one contiguous range of a buffer all ranks hold", i.e. an all-gather with
// ragged pieces.  xGMI on MI355X is a full mesh of point-to-point links (7 links per GPU), so the exchange is issued as ONE group of
// direct ncclSend / ncclRecv pairs -- every slab travels its own link straight into its final place in the peer's padded plane, no
// staging copy, no ring hops; with equal pieces and nothing but the gather to do the same group is what ncclAllGather would schedule.
//
// The list of transfers is built by pure host functions (svthip_*_plan) that need no device: the CPU tests execute the very same
// plan over gloo, so the partition and the offsets are covered without a multi-GPU node.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <new>

#include "../../include/svtav1_hip.h"

static_assert(SVTHIP_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");

struct svthip_comm {
    svthip_ctx* ctx;
    ncclComm_t nccl;
    int32_t rank, world;
};

namespace {

thread_local char g_comm_err[256] = "";

int32_t cfail(int32_t code, const char* what, const char* detail)
{
    snprintf(g_comm_err, sizeof(g_comm_err), "%s: %s", what, detail);
    return code;
}
#define NCCL_TRY(expr)                                                                    \
    do {                                                                                  \
        ncclResult_t r_ = (expr);                                                         \
        if (r_ != ncclSuccess) return cfail(SVTHIP_ERR_DEVICE, #expr, ncclGetErrorString(r_)); \
    } while (0)
#define HIPC_TRY(expr)                                                                   \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) return cfail(SVTHIP_ERR_DEVICE, #expr, hipGetErrorString(e_)); \
    } while (0)

// chroma geometry of PadRefAndSetFlags (Codec/EbEncDecProcess.c:1148-1204): 4:2:0, everything >> 1
struct PlaneGeom {
    uint32_t stride, width, height, pad_x, pad_y;
};
PlaneGeom plane_geom(const svthip_recon_picture& p, int plane)
{
    if (plane == 0) return PlaneGeom{p.stride_y, p.width, p.height, p.origin_x, p.origin_y};
    return PlaneGeom{plane == 1 ? p.stride_cb : p.stride_cr, (uint32_t)p.width >> 1, (uint32_t)p.height >> 1, (uint32_t)p.origin_x >> 1,
                     (uint32_t)p.origin_y >> 1};
}

int32_t check_picture(const svthip_recon_picture* p)
{
    if (!p) return cfail(SVTHIP_ERR_BAD_PARAMETER, "recon picture", "null");
    if (p->sample_bytes != 1 && p->sample_bytes != 2) return cfail(SVTHIP_ERR_BAD_PARAMETER, "recon picture", "sample_bytes must be 1 or 2");
    if (!p->width || !p->height || (p->width & 1) || (p->height & 1)) return cfail(SVTHIP_ERR_BAD_PARAMETER, "recon picture", "dimensions must be even and non-zero");
    for (int pl = 0; pl < (p->cb ? 3 : 1); pl++) {
        const PlaneGeom g = plane_geom(*p, pl);
        if (g.stride < g.width + 2 * g.pad_x) return cfail(SVTHIP_ERR_BAD_PARAMETER, "recon picture", "stride smaller than width + 2 * origin_x");
    }
    return SVTHIP_OK;
}

}  // namespace

extern "C" {

const char* svthip_comm_last_error(void) { return g_comm_err; }

void svthip_shard_range(uint32_t n_units, int32_t world, int32_t rank, uint32_t* first, uint32_t* count)
{
    // contiguous, balanced to one unit: the first n_units % world ranks take one more
    if (world < 1) world = 1;
    if (rank < 0) rank = 0;
    if (rank >= world) rank = world - 1;
    const uint32_t base = n_units / (uint32_t)world, extra = n_units % (uint32_t)world;
    const uint32_t r = (uint32_t)rank;
    if (first) *first = r * base + (r < extra ? r : extra);
    if (count) *count = base + (r < extra ? 1u : 0u);
}

void svthip_recon_slab_rows(uint32_t height, int32_t world, int32_t rank, uint32_t* first_row, uint32_t* n_rows)
{
    uint32_t f, c;
    svthip_shard_range((height + 63u) / 64u, world, rank, &f, &c);
    const uint32_t y0 = f * 64u < height ? f * 64u : height;
    const uint32_t y1 = (f + c) * 64u < height ? (f + c) * 64u : height;
    if (first_row) *first_row = y0;
    if (n_rows) *n_rows = y1 - y0;
}

int32_t svthip_recon_exchange_plan(const svthip_recon_picture* pic, int32_t world, int32_t rank, svthip_xfer* out, uint32_t max_xfers,
                                   uint32_t* n_xfers)
{
    int32_t rc = check_picture(pic);
    if (rc) return rc;
    if (world < 1 || rank < 0 || rank >= world || !n_xfers) return cfail(SVTHIP_ERR_BAD_PARAMETER, "exchange plan", "bad rank / world");
    const int n_planes = pic->cb ? 3 : 1;  // luma only when the chroma pointers are null
    uint32_t n = 0;
    // per plane and peer: the peer's slab comes in, this rank's slab goes out; rows are whole strides, so a slab is one byte range
    for (int pl = 0; pl < n_planes; pl++) {
        const PlaneGeom g = plane_geom(*pic, pl);
        const uint32_t sub = pl ? 1u : 0u;
        uint32_t my0, myn;
        svthip_recon_slab_rows(pic->height, world, rank, &my0, &myn);
        const uint64_t row_bytes = (uint64_t)g.stride * pic->sample_bytes;
        for (int32_t peer = 0; peer < world; peer++) {
            if (peer == rank) continue;
            uint32_t p0, pn;
            svthip_recon_slab_rows(pic->height, world, peer, &p0, &pn);
            // chroma rows of a luma slab [y0, y0 + n): [y0 >> 1, (y0 + n) >> 1) -- slab boundaries are multiples of 64 or the (even) height
            const uint32_t r0 = p0 >> sub, rn = ((p0 + pn) >> sub) - r0, s0 = my0 >> sub, sn = ((my0 + myn) >> sub) - s0;
            if (rn) {
                if (out && n < max_xfers) out[n] = svthip_xfer{peer, (uint32_t)pl, 0u, (uint64_t)(g.pad_y + r0) * row_bytes, (uint64_t)rn * row_bytes};
                n++;
            }
            if (sn) {
                if (out && n < max_xfers) out[n] = svthip_xfer{peer, (uint32_t)pl, 1u, (uint64_t)(g.pad_y + s0) * row_bytes, (uint64_t)sn * row_bytes};
                n++;
            }
        }
    }
    *n_xfers = n;
    if (out && n > max_xfers) return cfail(SVTHIP_ERR_INSUFFICIENT_RESOURCES, "exchange plan", "transfer list too short");
    return SVTHIP_OK;
}

int32_t svthip_me_gather_plan(uint32_t n_sb_total, uint32_t n_jobs, uint32_t record_bytes, int32_t world, int32_t rank, svthip_xfer* out,
                              uint32_t max_xfers, uint32_t* n_xfers)
{
    if (world < 1 || rank < 0 || rank >= world || !n_xfers || !record_bytes) return cfail(SVTHIP_ERR_BAD_PARAMETER, "gather plan", "bad argument");
    uint32_t my0, myn, n = 0;
    svthip_shard_range(n_sb_total, world, rank, &my0, &myn);
    // `plane` = job; receives land in the full array [n_jobs][n_sb_total][record], sends leave the local array [n_jobs][count][record]
    for (uint32_t j = 0; j < n_jobs; j++)
        for (int32_t peer = 0; peer < world; peer++) {
            if (peer == rank) continue;
            uint32_t p0, pn;
            svthip_shard_range(n_sb_total, world, peer, &p0, &pn);
            if (pn) {
                if (out && n < max_xfers) out[n] = svthip_xfer{peer, j, 0u, ((uint64_t)j * n_sb_total + p0) * record_bytes, (uint64_t)pn * record_bytes};
                n++;
            }
            if (myn) {
                if (out && n < max_xfers) out[n] = svthip_xfer{peer, j, 1u, (uint64_t)j * myn * record_bytes, (uint64_t)myn * record_bytes};
                n++;
            }
        }
    *n_xfers = n;
    if (out && n > max_xfers) return cfail(SVTHIP_ERR_INSUFFICIENT_RESOURCES, "gather plan", "transfer list too short");
    return SVTHIP_OK;
}

int32_t svthip_comm_get_unique_id(uint8_t* id)
{
    if (!id) return cfail(SVTHIP_ERR_BAD_PARAMETER, "svthip_comm_get_unique_id", "null id");
    ncclUniqueId u;
    NCCL_TRY(ncclGetUniqueId(&u));
    memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
    return SVTHIP_OK;
}

int32_t svthip_comm_create(svthip_ctx* ctx, const uint8_t* id, int32_t rank, int32_t world, svthip_comm** out)
{
    if (!ctx || !out || world < 1 || rank < 0 || rank >= world) return cfail(SVTHIP_ERR_BAD_PARAMETER, "svthip_comm_create", "bad argument");
    *out = nullptr;
    if (world > 1 && !id) return cfail(SVTHIP_ERR_BAD_PARAMETER, "svthip_comm_create", "null id");
    if (svthip_synchronize(ctx) != SVTHIP_OK) return cfail(SVTHIP_ERR_DEVICE, "svthip_comm_create", svthip_last_error());  // device current
    svthip_comm* c = new (std::nothrow) svthip_comm();
    if (!c) return cfail(SVTHIP_ERR_INSUFFICIENT_RESOURCES, "svthip_comm_create", "out of host memory");
    c->ctx = ctx;
    c->rank = rank;
    c->world = world;
    c->nccl = nullptr;
    if (world > 1) {  // a single rank never touches RCCL: its exchange is the local part only
        ncclUniqueId u;
        memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
        ncclResult_t r = ncclCommInitRank(&c->nccl, world, u, rank);
        if (r != ncclSuccess) {
            delete c;
            return cfail(SVTHIP_ERR_DEVICE, "ncclCommInitRank", ncclGetErrorString(r));
        }
    }
    *out = c;
    return SVTHIP_OK;
}

void svthip_comm_destroy(svthip_comm* c)
{
    if (!c) return;
    (void)svthip_synchronize(c->ctx);
    if (c->nccl) (void)ncclCommDestroy(c->nccl);
    delete c;
}

int32_t svthip_comm_rank(const svthip_comm* c) { return c ? c->rank : -1; }
int32_t svthip_comm_world(const svthip_comm* c) { return c ? c->world : 0; }

int32_t svthip_recon_exchange_dev(svthip_comm* c, const svthip_recon_picture* pic, void* stream)
{
    if (!c) return cfail(SVTHIP_ERR_BAD_PARAMETER, "svthip_recon_exchange_dev", "null communicator");
    int32_t rc = check_picture(pic);
    if (rc) return rc;
    if (!pic->y) return cfail(SVTHIP_ERR_BAD_PARAMETER, "svthip_recon_exchange_dev", "null luma plane");
    if ((pic->cb == nullptr) != (pic->cr == nullptr)) return cfail(SVTHIP_ERR_BAD_PARAMETER, "svthip_recon_exchange_dev", "cb and cr must both be given or both be null");
    hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)svthip_stream(c->ctx);
    uint8_t* base[3] = {static_cast<uint8_t*>(pic->y), static_cast<uint8_t*>(pic->cb), static_cast<uint8_t*>(pic->cr)};
    const int n_planes = pic->cb ? 3 : 1;
    if (c->world > 1) {
        svthip_xfer plan[3 * 2 * 64];
        uint32_t n = 0;
        if (c->world > 64) return cfail(SVTHIP_ERR_BAD_PARAMETER, "svthip_recon_exchange_dev", "more than 64 ranks");
        if ((rc = svthip_recon_exchange_plan(pic, c->world, c->rank, plan, 3 * 2 * 64, &n))) return rc;
        NCCL_TRY(ncclGroupStart());
        for (uint32_t i = 0; i < n; i++) {
            const svthip_xfer& x = plan[i];
            ncclResult_t r = x.send ? ncclSend(base[x.plane] + x.offset, x.bytes, ncclUint8, x.peer, c->nccl, s)
                                    : ncclRecv(base[x.plane] + x.offset, x.bytes, ncclUint8, x.peer, c->nccl, s);
            if (r != ncclSuccess) {
                (void)ncclGroupEnd();
                return cfail(SVTHIP_ERR_DEVICE, x.send ? "ncclSend" : "ncclRecv", ncclGetErrorString(r));
            }
        }
        NCCL_TRY(ncclGroupEnd());
    }
    // PadRefAndSetFlags: generate_padding / generate_padding16_bit of Y, Cb, Cr, redundantly on every rank
    for (int pl = 0; pl < n_planes; pl++) {
        const PlaneGeom g = plane_geom(*pic, pl);
        rc = svthip_pad_plane_dev(c->ctx, base[pl], g.stride, g.width, g.height, g.pad_x, g.pad_y, pic->sample_bytes, s);
        if (rc) return cfail(rc, "svthip_pad_plane_dev", svthip_last_error());
    }
    return SVTHIP_OK;
}

int32_t svthip_me_gather_results_dev(svthip_comm* c, const void* d_local, void* d_full, uint32_t n_jobs, uint32_t n_sb_total, uint32_t record_bytes,
                                     void* stream)
{
    if (!c || !d_full || !record_bytes) return cfail(SVTHIP_ERR_BAD_PARAMETER, "svthip_me_gather_results_dev", "bad argument");
    if (n_jobs == 0 || n_sb_total == 0) return SVTHIP_OK;
    hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)svthip_stream(c->ctx);
    uint32_t my0, myn;
    svthip_shard_range(n_sb_total, c->world, c->rank, &my0, &myn);
    if (myn && !d_local) return cfail(SVTHIP_ERR_BAD_PARAMETER, "svthip_me_gather_results_dev", "null local results");
    // this rank's own rows: [n_jobs][count][record] -> [n_jobs][n_sb_total][record] at its range
    if (myn && static_cast<const uint8_t*>(d_local) != static_cast<uint8_t*>(d_full) + (size_t)my0 * record_bytes)
        HIPC_TRY(hipMemcpy2DAsync(static_cast<uint8_t*>(d_full) + (size_t)my0 * record_bytes, (size_t)n_sb_total * record_bytes, d_local,
                                  (size_t)myn * record_bytes, (size_t)myn * record_bytes, n_jobs, hipMemcpyDeviceToDevice, s));
    if (c->world > 1) {
        uint32_t n = 0;
        int32_t rc;
        if ((rc = svthip_me_gather_plan(n_sb_total, n_jobs, record_bytes, c->world, c->rank, nullptr, 0, &n))) return rc;
        svthip_xfer* plan = new (std::nothrow) svthip_xfer[n ? n : 1];
        if (!plan) return cfail(SVTHIP_ERR_INSUFFICIENT_RESOURCES, "svthip_me_gather_results_dev", "out of host memory");
        rc = svthip_me_gather_plan(n_sb_total, n_jobs, record_bytes, c->world, c->rank, plan, n, &n);
        ncclResult_t r = rc ? ncclSuccess : ncclGroupStart();
        for (uint32_t i = 0; !rc && r == ncclSuccess && i < n; i++) {
            const svthip_xfer& x = plan[i];
            r = x.send ? ncclSend(static_cast<const uint8_t*>(d_local) + x.offset, x.bytes, ncclUint8, x.peer, c->nccl, s)
                       : ncclRecv(static_cast<uint8_t*>(d_full) + x.offset, x.bytes, ncclUint8, x.peer, c->nccl, s);
        }
        if (!rc) {
            const ncclResult_t re = ncclGroupEnd();
            if (r == ncclSuccess) r = re;
        }
        delete[] plan;
        if (rc) return rc;
        if (r != ncclSuccess) return cfail(SVTHIP_ERR_DEVICE, "RCCL send/recv group", ncclGetErrorString(r));
    }
    return SVTHIP_OK;
}

}  // extern "C"
