#!/usr/bin/env python3
"""Times AV1 film-grain synthesis on one 1920 x 1080 and one 3840 x 2160 picture at 8 and at 10 bits: svthip_film_grain_tables_dev alone
(one workgroup; the picture's size does not enter), the frame pass alone (tables given), the one-call form (both launches), and next to
them in the same run a device-to-device copy of the same three planes (the frame pass moves those bytes plus cache-resident table reads)
and the download plus upload of the three planes to pageable host memory that a host-side synthesis would cost.

    python tools/film_grain_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/film_grain_probe.py --cpu [--out FILE]                the CPU yardstick (build container only, where the reference exists)
    python tools/film_grain_probe.py --resources FILE                  registers, LDS and scratch of the kernels from the compiler's remarks

Device times are microseconds per call: the median over N samples, each the mean of back-to-back calls queued behind a sleep kernel, as
tools/probe_common.py: timed takes them; bytes are the three planes read plus written, and GB/s is bytes over that time.  Parameters: lag 3,
overlap on, 14 / 10 / 10 scaling points (the most work per table and per sample).  --cpu times the reference's own av1_add_film_grain on
one thread through the fixture driver (tests/golden/ref_film_grain_driver.c): microseconds per picture, best of three runs of 3 calls; it
is measured on the build machine's CPU, not next to the device.  One JSON line per row, appended to --out.  For a kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/film_grain_probe.py --iters 2"""
import argparse
import tempfile

import numpy as np

from probe_common import add_common_args, as_dev, emit, host_timed, open_stream, resources, timed, write_rows  # sets the import path

SIZES = ((1920, 1080), (3840, 2160))


def probe_params():
    import film_grain_util as fu
    p = dict(fu.PARAM_SETS[4])      # 14 / 10 / 3 points, overlap, full range
    p.update(fu._coeffs(11, 3, -10, 10, (30, -30)))
    p["ar_coeff_lag"], p["scaling_points_cr"], p["num_cr_points"] = 3, p["scaling_points_cb"], p["num_cb_points"]
    return p


def cpu_yardstick(lines):
    import film_grain_util as fu
    import make_golden_film_grain as gen
    assert gen.reference_available(), "the CPU yardstick needs the reference sources and oracle/_ref/obj_all"
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(tmp)
        for w, h in SIZES:
            for bd in fu.BIT_DEPTHS:
                t = min(L.drv_fg_time(gen._params(probe_params(), bd), w, h, bd, 3) for _ in range(3)) / 3
                emit(lines, {"entry": "reference av1_add_film_grain, 1 picture, 1 thread", "kind": "cpu, build container, host clock", "width": w,
                             "height": h, "bit_depth": bd, "us": round(t * 1e6, 1)})


def device_times(lines, iters):
    import torch

    import film_grain_util as fu
    import svtav1_hip
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    p = probe_params()
    params = svtav1_hip.film_grain_params(**p)

    def report(name, fn, reps, w, h, bd, nbytes, kind="device events", us=None, **more):
        us = timed(torch, fn, iters, reps).median if us is None else us
        row = {"entry": name, "kind": kind, "width": w, "height": h, "bit_depth": bd, "us": round(us, 1), "bytes": nbytes, **more}
        if nbytes:
            row["GB_per_s"] = round(nbytes / us / 1e3, 1)
        emit(lines, row)
        return us

    for w, h in SIZES:
        for bd in fu.BIT_DEPTHS:
            planes = fu.source_planes(w, h, bd, 0)
            d_src = [as_dev(torch, a) for a in planes]
            d_dst = [torch.zeros_like(t) for t in d_src]
            d_tab = torch.zeros(fu.TABLES_INT16, dtype=torch.int16, device="cuda:0")
            src, dst, strides = [t.data_ptr() for t in d_src], [t.data_ptr() for t in d_dst], [w, w // 2, w // 2]
            nbytes = 2 * sum(t.numel() for t in d_src)
            add = (lambda tab: ctx.add_film_grain_dev(params, src, strides, dst, strides, w, h, tab, stream=stream)) if bd == 8 else \
                (lambda tab: ctx.highbd_add_film_grain_dev(params, src, strides, dst, strides, w, h, bd, tab, stream=stream))
            t_tab = report("film_grain_tables (lag 3)", lambda: ctx.film_grain_tables_dev(params, bd, d_tab.data_ptr(), stream=stream), 10, w, h, bd, 0)
            t_frame = report("add_film_grain, tables given", lambda: add(d_tab.data_ptr()), 10, w, h, bd, nbytes)
            # correctness of what was timed
            torch.cuda.synchronize()
            want = fu.add_film_grain(p, bd, *planes)
            assert all(np.array_equal(t.cpu().numpy().view(a.dtype).reshape(a.shape), a) for t, a in zip(d_dst, want)), "the timed frame pass differs"
            report("add_film_grain, one call (tables + frame)", lambda: add(None), 10, w, h, bd, nbytes)
            t_copy = timed(torch, lambda: [d.copy_(s) for d, s in zip(d_dst, d_src)], iters, 10).median
            report("yardstick: device-to-device copy of the three planes", None, 10, w, h, bd, nbytes, us=t_copy, frame_over_copy=round(t_frame / t_copy, 2),
                   tables_over_frame=round(t_tab / t_frame, 2))
            host = [torch.zeros(t.numel(), dtype=torch.uint8) for t in d_src]

            def down_and_up():
                for hst, t in zip(host, d_src):
                    hst.copy_(t)
                for hst, t in zip(host, d_dst):
                    t.copy_(hst)
                torch.cuda.synchronize()

            report("yardstick: download plus upload of the three planes, pageable host memory", None, 0, w, h, bd, nbytes,
                   kind="host clock around synchronous copies", us=host_timed(down_and_up, iters, torch.cuda.synchronize).median)
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 7, cpu=True, resources=True)
    a = ap.parse_args()
    lines = []
    if a.resources:
        return resources("fg_grain.hip", a.resources, spill=True)
    if a.cpu:
        cpu_yardstick(lines)
    else:
        device_times(lines, a.iters)
    write_rows(a.out, lines)


if __name__ == "__main__":
    main()
