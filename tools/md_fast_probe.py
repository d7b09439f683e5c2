#!/usr/bin/env python3
"""Times mode decision's fast loop for the candidates of one 1920 x 1080 picture at three luma sizes, 8x8, 32x32 and 64x64, each with
has_uv and six candidates a block: svthip_md_fast_cost_batch_dev (the three SADs and the fast cost of every candidate, one launch) and
svthip_md_fast_pick_batch_dev (the buffer walk and PreModeDecision of every block, one launch over the same groups).  Next to them in the
same run, two yardsticks: the device-to-host download of the same prediction tiles (the six candidate pictures, Y, Cb and Cr) to pageable
host memory, which is what a host-side SAD costs before it starts, and a device-to-device copy of the bytes the SAD launch must read (the
tiles and the source picture once).

    python tools/md_fast_probe.py [--iters N] [--out FILE]      device times (needs a GPU)
    python tools/md_fast_probe.py --resources FILE              registers, LDS and scratch of the kernels from the compiler's remarks

The prediction pool holds candidate c of the block at (x, y) at (x, c * 1080 + y): six pictures stacked.  Device times are microseconds
per call: the median over N samples, each the mean of back-to-back calls queued behind a sleep kernel, as tools/probe_common.py: timed takes
them; GB/s is the bytes the launch must read over that time.  What was timed is compared with numpy before it is reported.  One JSON line
per row, appended to --out.  For a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/md_fast_probe.py --iters 2"""
import argparse

import numpy as np

from probe_common import add_common_args, as_dev, emit, host_timed, open_stream, resources, timed, write_rows  # sets the import path

W, H, CANDIDATES = 1920, 1080, 6
SIZES = (8, 32, 64)


def block_sads(src, pool, size):
    """[blocks][candidates] SAD of every size x size block of a plane against the six stacked candidate pictures"""
    h, w = src.shape
    ny, nx = h // size, w // size
    d = np.abs(pool.reshape(CANDIDATES, h, w).astype(np.int32) - src.astype(np.int32))[:, :ny * size, :nx * size]
    return d.reshape(CANDIDATES, ny, size, nx, size).sum(axis=(2, 4)).reshape(CANDIDATES, ny * nx).T


def device_times(lines, iters):
    import torch

    import md_fast_util as mu
    import svtav1_hip
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    luma = ((np.sin(xx / 17.0) + np.cos(yy / 11.0)) * 60 + 128 + rng.integers(-6, 7, (H, W))).clip(0, 255).astype(np.uint8)
    src = [luma, luma[::2, ::2].copy(), luma[1::2, 1::2].copy()]
    pool = [np.concatenate([(p.astype(np.int32) + rng.integers(-3 * (c + 1), 3 * (c + 1) + 1, p.shape)).clip(0, 255).astype(np.uint8)
                            for c in range(CANDIDATES)]) for p in src]
    d_src, d_pool = [torch.from_numpy(p).to("cuda:0") for p in src], [torch.from_numpy(p).to("cuda:0") for p in pool]
    planes = []
    for d, stride in ((d_src, W), (d_pool, W)):
        p = svtav1_hip.InterPlanes()
        p.y, p.cb, p.cr = (t.data_ptr() for t in d)
        p.y_stride, p.c_stride = stride, stride // 2
        planes.append(p)
    tile_bytes, src_bytes = sum(p.nbytes for p in pool), sum(p.nbytes for p in src)

    def report(name, us, size, n, nbytes, kind="device events", **more):
        row = {"entry": name, "kind": kind, "width": W, "height": H, "block": size if isinstance(size, str) else f"{size}x{size}", "candidates": n, "us": round(us, 1), "bytes": nbytes, **more}
        if nbytes:
            row["GB_per_s"] = round(nbytes / us / 1e3, 1)
        emit(lines, row)

    # the yardsticks do not depend on the block size
    d_copy = [torch.empty_like(t) for t in d_pool + d_src]
    t_copy = timed(torch, lambda: [d.copy_(s) for d, s in zip(d_copy, d_pool + d_src)], iters, 10).median
    host = [torch.empty(t.shape, dtype=torch.uint8) for t in d_pool]
    t_down = host_timed(lambda: ([hst.copy_(t) for hst, t in zip(host, d_pool)], torch.cuda.synchronize()), iters, torch.cuda.synchronize).median

    for size in SIZES:
        nx, ny = W // size, H // size
        n_blocks, n = nx * ny, nx * ny * CANDIDATES
        desc = np.zeros((n_blocks, CANDIDATES), mu.DESC_DTYPE)
        bx, by = np.meshgrid(np.arange(nx) * size, np.arange(ny) * size)
        for c in range(CANDIDATES):
            desc["src_x"][:, c], desc["src_y"][:, c] = bx.reshape(-1), by.reshape(-1)
            desc["pred_x"][:, c], desc["pred_y"][:, c] = bx.reshape(-1), by.reshape(-1) + c * H
            desc["flags"][:, c] = mu.TYPE_INTER if c & 1 else 0
        desc["rate"] = rng.integers(200, 6000, desc.shape)
        desc["merge_rate"], desc["lambda_"], desc["has_uv"] = mu.NO_MERGE, 1500, 1
        desc = desc.reshape(-1)
        groups = np.zeros(n_blocks, mu.GROUP_DTYPE)
        groups["first"], groups["count"], groups["buffer_total_count"], groups["buffer_width"] = np.arange(n_blocks) * CANDIDATES, CANDIDATES, 3, 13
        d_desc, d_groups = as_dev(torch, desc), as_dev(torch, groups)
        d_result = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
        d_pick = torch.zeros(n_blocks * 32, dtype=torch.uint8, device="cuda:0")
        cost = lambda: ctx.md_fast_cost_batch_dev(planes[0], planes[1], d_desc.data_ptr(), n, size, size, d_result.data_ptr(), stream=stream)  # noqa: E731
        pick = lambda: ctx.md_fast_pick_batch_dev(d_result.data_ptr(), d_desc.data_ptr(), n, d_groups.data_ptr(), n_blocks, d_pick.data_ptr(),  # noqa: E731
                                                  stream=stream)
        t_cost = timed(torch, cost, iters, 10).median
        t_pick = timed(torch, pick, iters, 10).median
        # correctness of what was timed
        torch.cuda.synchronize()
        got = d_result.cpu().numpy().view(mu.RESULT_DTYPE)
        luma_sad = block_sads(src[0], pool[0], size).reshape(-1)
        chroma_sad = (block_sads(src[1], pool[1], size // 2) + block_sads(src[2], pool[2], size // 2)).reshape(-1)
        assert np.array_equal(got["luma"], luma_sad) and np.array_equal(got["chroma"], chroma_sad), "the timed SADs differ"
        want_cost = ((desc["rate"].astype(np.uint64) * np.uint64(1500) + np.uint64(256)) >> np.uint64(9)) + ((luma_sad + chroma_sad).astype(np.uint64) << np.uint64(7))
        assert np.array_equal(got["cost"], want_cost), "the timed costs differ"
        some = np.arange(0, n_blocks, max(1, n_blocks // 500))
        want_pick = mu.pick(got, desc, groups[some])[0]
        assert np.array_equal(d_pick.cpu().numpy().view(mu.PICK_DTYPE)[some], want_pick), "the timed picks differ"
        assert ctx.inter_pred_refused() == 0
        read = n_blocks * CANDIDATES * size * size * 3 // 2 + n_blocks * size * size * 3 // 2 + desc.nbytes
        report("md_fast_cost (3 SADs + cost per candidate)", t_cost, size, n, read, cost_over_copy=round(t_cost / t_copy, 2),
               download_over_cost=round(t_down / t_cost, 1))
        report("md_fast_pick (walk + PreModeDecision per block)", t_pick, size, n, 0, groups=n_blocks)
    report("yardstick: device-to-device copy of the six candidate pictures and the source picture", t_copy, "all", 0, tile_bytes + src_bytes)
    report("yardstick: download of the six candidate pictures to pageable host memory", t_down, "all", 0, tile_bytes, kind="host clock around synchronous copies")
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 7, resources=True)
    a = ap.parse_args()
    if a.resources:
        return resources("md_fast.hip", a.resources, spill=True)
    lines = []
    device_times(lines, a.iters)
    write_rows(a.out, lines)


if __name__ == "__main__":
    main()
