#!/usr/bin/env python3
"""Times the Wiener loop-restoration entries on a 1920 x 1080 picture (luma unit 256: 8 x 4 units; chroma 128), 8 and 10 bits: the
statistics of the three planes, the solve, one SSE trial of all units, the whole search (with the number of trials it took), and the frame
filter of the three planes.

    python tools/lr_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/lr_probe.py --cpu [--out FILE]                the CPU yardstick (build container only, where the reference exists)

Device times are microseconds: the median over N samples, each the mean of back-to-back calls queued behind a sleep kernel, as
tools/probe_common.py: timed takes them.  One JSON line per row; --out is overwritten.  The pictures are the synthetic ones of tests/golden/make_golden_lr.py.
--cpu times the reference's own search_norestore_seg + search_wiener_seg over the same pictures, one thread, through the fixture driver
(tests/golden/ref_lr_driver.c; leaf functions as the encoder dispatches them, AVX2): seconds per picture, best of three.
For a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/lr_probe.py --iters 3"""
import argparse
import functools
import json
import tempfile

import numpy as np

from probe_common import add_common_args, as_dev, emit, open_stream, timed, write_rows  # sets the import path

import make_golden_lr as gen  # noqa: E402

W, H = 1920, 1080


def cpu_yardstick(lines):
    assert gen.reference_available(), "the CPU yardstick needs the reference sources and oracle/_ref/obj_all"
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(tmp)
        for bd in (8, 10):
            cdef, dbk, src = gen.make_pictures(np.random.default_rng(bd), W, H, bd)
            R = gen.Reference(L, W, H, bd, cdef, dbk, src)
            t = min(L.drv_lr_time(None) for _ in range(3))
            R.close()
            emit(lines, {"entry": "reference search_norestore_seg + search_wiener_seg, 3 planes, 1 thread", "bit_depth": bd, "us": round(t * 1e6, 1)})


def device_times(lines, iters):
    import torch

    import svtav1_hip
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    dev = functools.partial(as_dev, torch)
    base, _ = svtav1_hip.lr_unit_geometry(W, H)
    n = base[3]

    def report(name, bd, fn, reps, **more):
        emit(lines, {"entry": name, "bit_depth": bd, "us": round(timed(torch, fn, iters, reps).median, 1), **more})

    for bd in (8, 10):
        planes = gen.make_pictures(np.random.default_rng(bd), W, H, bd)
        d = [[dev(p) for p in s] for s in planes]
        strides = [W, W // 2, W // 2]
        pic = svtav1_hip.make_lr_picture(W, H, [t.data_ptr() for t in d[0]], strides, [t.data_ptr() for t in d[1]], strides, [t.data_ptr() for t in d[2]],
                                         strides)
        d_out = [torch.zeros_like(t) for t in d[0]]
        work = torch.zeros(svtav1_hip.lr_workspace_bytes(n) // 8, dtype=torch.int64, device="cuda:0")
        d_M, d_H = torch.zeros(n * 49, dtype=torch.int64, device="cuda:0"), torch.zeros(n * 2401, dtype=torch.int64, device="cuda:0")
        d_avg, d_rej = torch.zeros(n, dtype=torch.int32, device="cuda:0"), torch.zeros(n, dtype=torch.int32, device="cuda:0")
        d_none, d_sse = torch.zeros(n, dtype=torch.int64, device="cuda:0"), torch.zeros(2 * n, dtype=torch.int64, device="cuda:0")
        d_taps, d_ntr = torch.zeros(16 * n, dtype=torch.int16, device="cuda:0"), torch.zeros(n, dtype=torch.int32, device="cuda:0")
        d_pending = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        d_type = torch.ones(n, dtype=torch.uint8, device="cuda:0")
        stats = lambda: ctx.av1_wiener_stats_dev(pic, 0, 3, d_M.data_ptr(), d_H.data_ptr(), d_avg.data_ptr(), d_none.data_ptr(), work.data_ptr(),  # noqa: E731
                                                 bit_depth=bd, stream=stream)

        def solve():
            ctx.wiener_solve_dev(d_M.data_ptr(), d_H.data_ptr(), 0, base[1], 7, d_taps.data_ptr(), d_rej.data_ptr(), stream=stream)
            ctx.wiener_solve_dev(d_M.data_ptr(), d_H.data_ptr(), base[1], n, 5, d_taps.data_ptr(), d_rej.data_ptr(), stream=stream)

        search = lambda: ctx.av1_search_wiener_dev(pic, 0, 3, work.data_ptr(), d_sse.data_ptr(), d_taps.data_ptr(), d_ntr.data_ptr(),  # noqa: E731
                                                   d_pending.data_ptr(), bit_depth=bd, stream=stream)
        report("wiener_stats (3 planes)", bd, stats, 5, units=n)
        report("wiener_solve (all units)", bd, solve, 5)
        report("wiener_trial_sse (all units, 3 planes)", bd,
               lambda: ctx.av1_wiener_trial_sse_dev(pic, 0, 3, d_taps.data_ptr(), d_none.data_ptr(), None, bit_depth=bd, stream=stream), 10)
        report("search_wiener (default step count)", bd, search, 2)
        torch.cuda.synchronize()
        ntr = d_ntr.cpu().numpy()
        lines[-1].update(trials_max=int(ntr.max()), trials_sum=int(ntr.sum()), pending=int(d_pending.cpu()[0]), rejected=int((d_sse.cpu().numpy()[1::2] == (1 << 63) - 1).sum()))
        print(json.dumps(lines[-1]), flush=True)
        report("loop_restoration_filter_frame (3 planes, all Wiener)", bd,
               lambda: ctx.av1_loop_restoration_filter_frame_dev(pic, [t.data_ptr() for t in d_out], strides, 0, 3, d_type.data_ptr(), d_taps.data_ptr(),
                                                                 bit_depth=bd, stream=stream), 10)
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 10, cpu=True)
    a = ap.parse_args()
    lines = []
    if a.cpu:
        cpu_yardstick(lines)
    else:
        device_times(lines, a.iters)
    write_rows(a.out, lines, append=False)


if __name__ == "__main__":
    main()
