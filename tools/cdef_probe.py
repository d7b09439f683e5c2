#!/usr/bin/env python3
"""Times the CDEF entries on a synthetic 1920 x 1080 picture (30 x 17 filter blocks), 8 and 10 bits: the strength search of all filter
blocks, the strength pick, the frame filter of the three planes with the search's own result, and, next to them, the two copies of the
three planes that a host CDEF between two device stages costs (device to pinned host memory and back, hipMemcpyAsync on the same stream);
then the search and the pick for grids with 128-wide blocks, on a grid of BLOCK_64X64 (the same 510 fbs) and on one of BLOCK_128X128
(135 wide fbs), with the existing pick on the same tables beside them.

    python tools/cdef_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/cdef_probe.py --cpu [--out FILE]                the CPU yardstick (build container only, where the reference exists)
    python tools/cdef_probe.py --resources FILE                  registers, LDS and scratch of the kernels from the code object's notes

Device times are microseconds: the median over N samples, each the mean of back-to-back calls queued behind a sleep kernel, as
tools/probe_common.py: timed takes them.  One JSON line per row, appended to --out.  The pictures are the synthetic ones of tests/golden/make_golden_cdef.py with 30 % of the cells skipped.
--cpu times the reference's own cdef_seg_search, finish_cdef_search and av1_cdef_frame over the same pictures, one thread, through the
fixture driver (tests/golden/ref_cdef_driver.c; leaf functions as the encoder dispatches them, AVX2, but the C mse_4x4_16bit): seconds per
picture, best of two.
For a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/cdef_probe.py --iters 2"""
import argparse
import functools
import tempfile

import numpy as np

from probe_common import add_common_args, as_dev, emit, open_stream, resources, timed, write_rows  # sets the import path

import make_golden_cdef as gen  # noqa: E402

W, H, QINDEX = 1920, 1080, 100


def pictures(bd):
    rng = np.random.default_rng(bd)
    dbk, src = gen.make_pictures(rng, W, H, bd)
    return dbk, src, (rng.random((H // 4, W // 4)) < 0.3).astype(np.uint8)


def cpu_yardstick(lines):
    assert gen.reference_available(), "the CPU yardstick needs the reference sources and oracle/_ref/obj_all"
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(tmp)
        for bd in (8, 10):
            dbk, src, skip = pictures(bd)
            R = gen.Reference(L, W, H, bd, dbk, src, skip)
            total, parts = min((R.time(QINDEX) for _ in range(2)), key=lambda t: t[0])
            R.close()
            for name, t in zip(("cdef_seg_search", "finish_cdef_search", "av1_cdef_frame"), parts):
                emit(lines, {"entry": f"reference {name}, 1 thread", "bit_depth": bd, "us": round(float(t) * 1e6, 1)})
            emit(lines, {"entry": "reference search + finish + frame, 1 thread", "bit_depth": bd, "us": round(total * 1e6, 1)})


def device_times(lines, iters):
    import torch

    import svtav1_hip
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    dev = functools.partial(as_dev, torch)
    nh, nv = svtav1_hip.cdef_filter_blocks(W, H)
    nfb = nh * nv

    def report(name, bd, fn, reps, **more):
        emit(lines, {"entry": name, "bit_depth": bd, "us": round(timed(torch, fn, iters, reps).median, 1), **more})

    for bd in (8, 10):
        dbk, src, skip = pictures(bd)
        d_dbk, d_src, d_skip = [dev(p) for p in dbk], [dev(p) for p in src], dev(skip)
        d_out = [torch.zeros_like(t) for t in d_dbk]
        strides = [W, W // 2, W // 2]
        pic = svtav1_hip.make_cdef_picture(W, H, [t.data_ptr() for t in d_dbk], strides, d_skip.data_ptr(), W // 4, [t.data_ptr() for t in d_src], strides,
                                           [t.data_ptr() for t in d_out], strides)
        d_mse = torch.zeros(2 * nfb * 64, dtype=torch.int64, device="cuda:0")
        d_cnt = torch.zeros(nfb, dtype=torch.uint8, device="cuda:0")
        d_res = torch.zeros(21, dtype=torch.int32, device="cuda:0")
        d_fbs = torch.zeros(nfb, dtype=torch.int8, device="cuda:0")
        pinned = [torch.zeros(t.shape, dtype=t.dtype).pin_memory() for t in d_dbk]
        torch.cuda.synchronize()
        report("cdef_search_mse (all fbs, 3 planes)", bd,
               lambda: ctx.av1_cdef_search_mse_dev(pic, QINDEX, d_mse.data_ptr(), d_cnt.data_ptr(), bit_depth=bd, stream=stream), 2, fbs=nfb)
        report("cdef_pick_strengths", bd,
               lambda: ctx.cdef_pick_strengths_dev(d_mse.data_ptr(), d_cnt.data_ptr(), nh, nv, QINDEX, bd, d_res.data_ptr(), d_fbs.data_ptr(), stream=stream), 2)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(svtav1_hip.CDEF_RESULT_DTYPE)[0]
        lines[-1].update(sb_count=int(res["sb_count"]), cdef_bits=int(res["cdef_bits"]))
        report("cdef_frame (3 planes, the search's result)", bd,
               lambda: ctx.av1_cdef_frame_dev(pic, d_res.data_ptr(), d_fbs.data_ptr(), 0, 3, bit_depth=bd, stream=stream), 5)
        report("cdef_search (search + pick, one call)", bd,
               lambda: ctx.av1_cdef_search_dev(pic, QINDEX, d_mse.data_ptr(), d_cnt.data_ptr(), d_res.data_ptr(), d_fbs.data_ptr(), bit_depth=bd,
                                               stream=stream), 2)

        # the entries for grids with 128-wide blocks: on a grid of 64X64 blocks (the same 510 fbs) and on one of 128X128 blocks (135 wide fbs)
        d_work = torch.zeros(svtav1_hip.cdef_search128_workspace_bytes(W, H) // 8, dtype=torch.int64, device="cuda:0")
        for label, sb_type in (("64X64 grid, 510 fbs", 12), ("128X128 grid, 135 wide fbs", 15)):
            grid = np.zeros((H // 4, W // 4), svtav1_hip.LF_MI_DTYPE)
            grid["sb_type"] = sb_type
            d_mi = dev(grid)
            torch.cuda.synchronize()
            report(f"cdef_search_mse128 ({label})", bd,
                   lambda: ctx.av1_cdef_search_mse128_dev(pic, QINDEX, d_mse.data_ptr(), d_cnt.data_ptr(), d_mi.data_ptr(), W // 4, d_work.data_ptr(), bit_depth=bd,
                                                          stream=stream), 2, fbs=nfb)
            report(f"cdef_pick_strengths128 ({label})", bd,
                   lambda: ctx.cdef_pick_strengths128_dev(d_mse.data_ptr(), d_cnt.data_ptr(), nh, nv, QINDEX, bd, d_res.data_ptr(), d_fbs.data_ptr(), d_mi.data_ptr(),
                                                          W // 4, stream=stream), 2)
            torch.cuda.synchronize()
            res = d_res.cpu().numpy().view(svtav1_hip.CDEF_RESULT_DTYPE)[0]
            lines[-1].update(sb_count=int(res["sb_count"]), cdef_bits=int(res["cdef_bits"]))
            report(f"cdef_pick_strengths on the same tables ({label})", bd,
                   lambda: ctx.cdef_pick_strengths_dev(d_mse.data_ptr(), d_cnt.data_ptr(), nh, nv, QINDEX, bd, d_res.data_ptr(), d_fbs.data_ptr(), stream=stream), 2,
                   sb_count=int(res["sb_count"]))

        def copies():
            for h, d in zip(pinned, d_dbk):
                h.copy_(d, non_blocking=True)
            for h, d in zip(pinned, d_out):
                d.copy_(h, non_blocking=True)

        report("the two plane copies a host CDEF costs (3 planes down, 3 up, pinned)", bd, copies, 5, bytes=2 * sum(t.numel() for t in d_dbk))
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 5, cpu=True, resources=True)
    a = ap.parse_args()
    lines = []
    if a.resources:
        return resources("cf_cdef.hip", a.resources)
    if a.cpu:
        cpu_yardstick(lines)
    else:
        device_times(lines, a.iters)
    write_rows(a.out, lines)


if __name__ == "__main__":
    main()
