#!/usr/bin/env python3
"""Times the self-guided loop-restoration entries on a 1920 x 1080 picture (luma unit 256: 8 x 4 units; chroma 128), 8 and 10 bits: the
whole search of the three planes (with the number of trials its walks took), the SSE trial of all units, and the frame filter with every
unit RESTORE_SGRPROJ.

    python tools/lr_sgr_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/lr_sgr_probe.py --cpu [--out FILE]                the CPU yardstick (build container only, where the reference exists)

Device times are microseconds: the median over N samples, each the mean of back-to-back calls queued behind a sleep kernel, as
tools/probe_common.py: timed takes them.  One JSON line per row; --out is overwritten.  The pictures are the synthetic ones of tests/golden/make_golden_lr.py.
--cpu times the reference's own search_sgrproj_seg over the same pictures, one thread, through the fixture driver
(tests/golden/ref_lr_sgr_driver.c; leaf functions as the encoder dispatches them, AVX2): seconds per picture, best of two.
For a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/lr_sgr_probe.py --iters 2"""
import argparse
import functools
import json
import tempfile

import numpy as np

from probe_common import add_common_args, as_dev, emit, open_stream, timed, write_rows  # sets the import path

import make_golden_lr as gen  # noqa: E402

W, H = 1920, 1080


def cpu_yardstick(lines):
    import make_golden_lr_sgr as gen_sgr
    assert gen.reference_available(), "the CPU yardstick needs the reference sources and oracle/_ref/obj_all"
    with tempfile.TemporaryDirectory() as tmp:
        L = gen_sgr.build_driver(tmp)
        for bd in (8, 10):
            cdef, dbk, src = gen.make_pictures(np.random.default_rng(bd), W, H, bd)
            R = gen.Reference(L, W, H, bd, cdef, dbk, src)
            t = min(L.drv_sgr_time() for _ in range(2))
            R.close()
            emit(lines, {"entry": "reference search_sgrproj_seg, 3 planes, 1 thread", "bit_depth": bd, "us": round(t * 1e6, 1)})


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
        work = torch.zeros(svtav1_hip.sgrproj_workspace_bytes(W, H) // 8 + 1, dtype=torch.int64, device="cuda:0")
        d_sgr, d_sse = torch.zeros(4 * n, dtype=torch.int32, device="cuda:0"), torch.zeros(n, dtype=torch.int64, device="cuda:0")
        d_det = torch.zeros(n * 16 * 80, dtype=torch.uint8, device="cuda:0")
        d_type = torch.full((n,), 2, dtype=torch.uint8, device="cuda:0")
        report("search_sgrproj (3 planes)", bd,
               lambda: ctx.av1_search_sgrproj_dev(pic, 0, 3, work.data_ptr(), d_sgr.data_ptr(), d_sse.data_ptr(), d_det.data_ptr(), bit_depth=bd, stream=stream),
               1, units=n)
        torch.cuda.synchronize()
        ntr = d_det.cpu().numpy().view(svtav1_hip.SGRPROJ_DETAIL_DTYPE)["n_trials"]
        lines[-1].update(trials_mean=round(float(ntr.mean()), 2), trials_max=int(ntr.max()), trials_sum=int(ntr.sum()))
        print(json.dumps(lines[-1]), flush=True)
        report("sgrproj_trial_sse (all units, 3 planes)", bd,
               lambda: ctx.av1_sgrproj_trial_sse_dev(pic, 0, 3, d_sgr.data_ptr(), d_sse.data_ptr(), None, bit_depth=bd, stream=stream), 5)
        report("lr_filter_frame (3 planes, all self-guided)", bd,
               lambda: ctx.av1_lr_filter_frame_dev(pic, [t.data_ptr() for t in d_out], strides, 0, 3, d_type.data_ptr(), None, d_sgr.data_ptr(), bit_depth=bd,
                                                   stream=stream), 5)
        if ctx.inter_pred_refused() != 0:
            raise SystemExit("a unit was refused")
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 5, cpu=True)
    a = ap.parse_args()
    lines = []
    if a.cpu:
        cpu_yardstick(lines)
    else:
        device_times(lines, a.iters)
    write_rows(a.out, lines, append=False)


if __name__ == "__main__":
    main()
