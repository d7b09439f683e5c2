#!/usr/bin/env python3
"""Times the restoration decision on the device against the host round trip it replaces, and the one-call restoration stage against its
four parts, at 1920 x 1080 (32 units a plane) and 3840 x 2160 (120 a plane), 8 bits, in one call.

    python tools/lr_finish_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/lr_finish_probe.py --cpu [--out FILE]                the CPU yardstick (build container only, where the reference exists)

Per size, the alternatives taken in turn within each sample:
  decision kernel, device        microseconds of svthip_rest_finish_search_dev, the median over N samples, each the mean of back-to-back calls
                                 queued behind a sleep kernel, as tools/probe_common.py: timed takes them
  decision, idle stream, host clock      enqueue on an idle stream and wait for it: what a caller that does wait would see
  round trip, host clock         what a host decision needs around it: hipMemcpyAsync of the four tables to pinned host memory, a stream
                                 synchronise, the upload of the unit types enqueued (and, second figure, completed).  No host computation
                                 in between: a floor for the host path
  the one-call entry and its four parts (Wiener search with its bound of trials, self-guided search, decision, frame filter), device times
The tables the decision reads are the searches' own results on the synthetic pictures of tests/golden/make_golden_lr.py; the rates are
ordinary ones (lr_finish_util.ORDINARY with rdmult 60000).
--cpu times the reference's rest_finish_search on tables of the same unit counts, one thread, through the fixture driver
(tests/golden/ref_lr_finish_driver.c): microseconds per picture, the mean of 1000 calls, best of three.
One JSON line per row; --out is overwritten, its folder made if it is not there.
For a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/lr_finish_probe.py --iters 2"""
import argparse
import functools
import os
import tempfile
import time

import numpy as np

from probe_common import add_common_args, as_dev, emit, open_stream, timed, write_rows  # sets the import path

import lr_finish_util as fu  # noqa: E402

SIZES = ((1920, 1080), (3840, 2160))
RATES = dict(fu.ORDINARY, rdmult=60000)


def cpu_yardstick(lines):
    import make_golden_lr_finish as gen
    from oracle.ref_driver import reference_available
    assert reference_available(), "the CPU yardstick needs the reference sources and oracle/_ref/obj_all"
    import svtav1_hip
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(tmp)
        for (w, h) in SIZES:
            us = svtav1_hip.lr_unit_sizes(w, h)
            counts = gen.open_geometry(L, w, h, us)
            base = fu.unit_base_of(counts)
            rng = np.random.default_rng(w)
            tables = fu.tables_of([[fu.random_unit(rng, p) for _ in range(counts[p])] for p in range(3)])
            ra, ub = fu.rates_array(RATES), np.array(base, np.int32)
            t = min(L.drv_finish_time(ra.ctypes.data, ub.ctypes.data, *[a.ctypes.data for a in tables], 1000) for _ in range(3)) / 1000
            L.drv_lr_close()
            emit(lines, {"entry": "reference rest_finish_search, 3 planes, 1 thread", "size": f"{w}x{h}", "units": base[3], "us": round(t * 1e6, 2)})


def device_times(lines, iters):
    import torch

    import make_golden_lr as gen
    import svtav1_hip
    ctx = svtav1_hip.Context(0)
    torch_stream, stream = open_stream(torch)
    dev = functools.partial(as_dev, torch)

    def report(name, size, us, **more):
        emit(lines, {"entry": name, "size": size, "us": round(us, 1), **more})

    for (w, h) in SIZES:
        size, bd = f"{w}x{h}", 8
        base, _ = svtav1_hip.lr_unit_geometry(w, h)
        n = base[3]
        planes = gen.make_pictures(np.random.default_rng(bd), w, h, bd)
        d = [[dev(p) for p in s] for s in planes]
        strides = [w, w // 2, w // 2]
        pic = svtav1_hip.make_lr_picture(w, h, [t.data_ptr() for t in d[0]], strides, [t.data_ptr() for t in d[1]], strides, [t.data_ptr() for t in d[2]],
                                         strides)
        d_out = [torch.zeros_like(t) for t in d[0]]
        out = [t.data_ptr() for t in d_out]
        zeros = lambda count, dt: torch.zeros(count, dtype=dt, device="cuda:0")  # noqa: E731
        work_w, work_s = zeros(svtav1_hip.lr_workspace_bytes(n) // 8 + 1, torch.int64), zeros(svtav1_hip.sgrproj_workspace_bytes(w, h) // 8 + 1, torch.int64)
        work = zeros(svtav1_hip.lr_pick_workspace_bytes(w, h) // 8 + 1, torch.int64)
        d_wsse, d_taps, d_ntr, d_pend = zeros(2 * n, torch.int64), zeros(16 * n, torch.int16), zeros(n, torch.int32), zeros(1, torch.int32)
        d_ssse, d_sgr = zeros(n, torch.int64), zeros(4 * n, torch.int32)
        d_type, d_res = zeros(n, torch.uint8), zeros(39, torch.int64)
        d_taps1, d_sgr1, d_type1, d_res1 = zeros(16 * n, torch.int16), zeros(4 * n, torch.int32), zeros(n, torch.uint8), zeros(39, torch.int64)
        host = [torch.zeros(t.numel(), dtype=t.dtype).pin_memory() for t in (d_wsse, d_taps, d_ssse, d_sgr)]
        h_type = torch.zeros(n, dtype=torch.uint8).pin_memory()
        torch.cuda.synchronize()
        on = {"bit_depth": bd, "stream": stream}

        wiener = lambda: ctx.av1_search_wiener_dev(pic, 0, 3, work_w.data_ptr(), d_wsse.data_ptr(), d_taps.data_ptr(), d_ntr.data_ptr(), d_pend.data_ptr(),  # noqa: E731
                                                   n_steps=0, **on)
        sgr = lambda: ctx.av1_search_sgrproj_dev(pic, 0, 3, work_s.data_ptr(), d_sgr.data_ptr(), d_ssse.data_ptr(), None, **on)  # noqa: E731
        decide = lambda: ctx.rest_finish_search_dev(RATES, base, 0, 3, d_wsse.data_ptr(), d_taps.data_ptr(), d_ssse.data_ptr(), d_sgr.data_ptr(),  # noqa: E731
                                                    d_type.data_ptr(), d_res.data_ptr(), stream=stream)
        filt = lambda: ctx.av1_lr_filter_frame_dev(pic, out, strides, 0, 3, d_type.data_ptr(), d_taps.data_ptr(), d_sgr.data_ptr(), **on)  # noqa: E731
        one = lambda: ctx.av1_pick_filter_restoration_dev(pic, RATES, work.data_ptr(), out, strides, d_type1.data_ptr(), d_taps1.data_ptr(), d_sgr1.data_ptr(),  # noqa: E731
                                                          d_res1.data_ptr(), **on)

        def idle_decision():
            t0 = time.perf_counter()
            decide()
            torch_stream.synchronize()
            return (time.perf_counter() - t0) * 1e6, 0.0

        def round_trip():
            t0 = time.perf_counter()
            for hst, dv in zip(host, (d_wsse, d_taps, d_ssse, d_sgr)):
                hst.copy_(dv, non_blocking=True)
            torch_stream.synchronize()
            d_type.copy_(h_type, non_blocking=True)
            t1 = time.perf_counter()
            torch_stream.synchronize()
            return (t1 - t0) * 1e6, (time.perf_counter() - t0) * 1e6

        wiener(), sgr()                       # the tables the decision reads
        torch_stream.synchronize()
        for _ in range(20):                   # warm both host paths
            idle_decision(), round_trip()
        samples = {"idle": [], "trip": []}
        for _ in range(max(iters, 1) * 40):   # the alternatives in turn
            samples["idle"].append(idle_decision())
            torch_stream.synchronize()
            h_type.copy_(d_type)              # the unit types the upload then carries, outside the timing
            samples["trip"].append(round_trip())
        report("decision kernel, device", size, timed(torch, decide, iters, 20).median, units=n)
        frame_types = d_res.cpu().numpy().view(svtav1_hip.rest_finish_result_dtype())["frame_type"].tolist()
        lines[-1]["frame_types"] = frame_types
        report("decision, idle stream, enqueue to completion, host clock", size, float(np.median([s[0] for s in samples["idle"]])))
        report("round trip: 4 downloads, synchronise, upload enqueued, host clock", size, float(np.median([s[0] for s in samples["trip"]])),
               upload_completed_us=round(float(np.median([s[1] for s in samples["trip"]])), 1))
        parts = {}
        for name, fn, reps in (("search_wiener (bound of trials)", wiener, 1), ("search_sgrproj", sgr, 1), ("decision", decide, 20), ("lr_filter_frame", filt, 5)):
            parts[name] = timed(torch, fn, iters, reps).median
            report("part: " + name, size, parts[name])
        report("sum of the four parts", size, sum(parts.values()))
        report("one-call entry", size, timed(torch, one, iters, 1).median)
        torch_stream.synchronize()
        same = all(torch.equal(a, b) for a, b in ((d_taps, d_taps1), (d_sgr, d_sgr1), (d_type, d_type1), (d_res, d_res1)))
        lines[-1]["same_outputs_as_parts"] = bool(same)
        if ctx.inter_pred_refused() != 0:
            raise SystemExit("a unit was refused")
        del d, d_out, work_w, work_s, work
        torch.cuda.empty_cache()
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
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        write_rows(a.out, lines, append=False)


if __name__ == "__main__":
    main()
