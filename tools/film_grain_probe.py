#!/usr/bin/env python3
"""Times AV1 film-grain synthesis on one 1920 x 1080 and one 3840 x 2160 picture at 8 and at 10 bits: svthip_film_grain_tables_dev alone
(one workgroup; the picture's size does not enter), the frame pass alone (tables given), the one-call form (both launches), and next to
them in the same run a device-to-device copy of the same three planes (the frame pass moves those bytes plus cache-resident table reads)
and the download plus upload of the three planes to pageable host memory that a host-side synthesis would cost.

    python tools/film_grain_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/film_grain_probe.py --cpu [--out FILE]                the CPU yardstick (build container only, where the reference exists)
    python tools/film_grain_probe.py --resources FILE                  registers, LDS and scratch of the kernels from the compiler's remarks

Device times are microseconds per call: the median over N samples, each the mean of back-to-back calls queued behind a sleep kernel, as
tools/inter_pred_probe.py takes them; bytes are the three planes read plus written, and GB/s is bytes over that time.  Parameters: lag 3,
overlap on, 14 / 10 / 10 scaling points (the most work per table and per sample).  --cpu times the reference's own av1_add_film_grain on
one thread through the fixture driver (tests/golden/ref_film_grain_driver.c): microseconds per picture, best of three runs of 3 calls; it
is measured on the build machine's CPU, not next to the device.  One JSON line per row, appended to --out.  For a kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/film_grain_probe.py --iters 2"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "svt-av1-1_amd", "python")]

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
                lines.append({"entry": "reference av1_add_film_grain, 1 picture, 1 thread", "kind": "cpu, build container, host clock", "width": w,
                              "height": h, "bit_depth": bd, "us": round(t * 1e6, 1)})
                print(json.dumps(lines[-1]), flush=True)


def device_times(lines, iters):
    import torch

    import film_grain_util as fu
    import svtav1_hip
    from inter_pred_probe import timed
    ctx = svtav1_hip.Context(0)
    torch_stream = torch.cuda.Stream()   # the default stream's handle is NULL, which the library reads as "the context's stream"
    torch.cuda.set_stream(torch_stream)
    stream = torch_stream.cuda_stream
    assert stream
    p = probe_params()
    params = svtav1_hip.film_grain_params(**p)

    def report(name, fn, reps, w, h, bd, nbytes, kind="device events", us=None, **more):
        us = timed(torch, fn, iters, reps) if us is None else us
        row = {"entry": name, "kind": kind, "width": w, "height": h, "bit_depth": bd, "us": round(us, 1), "bytes": nbytes, **more}
        if nbytes:
            row["GB_per_s"] = round(nbytes / us / 1e3, 1)
        lines.append(row)
        print(json.dumps(row), flush=True)
        return us

    for w, h in SIZES:
        for bd in fu.BIT_DEPTHS:
            planes = fu.source_planes(w, h, bd, 0)
            as_dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")  # noqa: E731
            d_src = [as_dev(a) for a in planes]
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
            t_copy = timed(torch, lambda: [d.copy_(s) for d, s in zip(d_dst, d_src)], iters, 10)
            report("yardstick: device-to-device copy of the three planes", None, 10, w, h, bd, nbytes, us=t_copy, frame_over_copy=round(t_frame / t_copy, 2),
                   tables_over_frame=round(t_tab / t_frame, 2))
            host = [torch.zeros(t.numel(), dtype=torch.uint8) for t in d_src]
            ts = []
            for _ in range(3 + iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for hst, t in zip(host, d_src):
                    hst.copy_(t)
                for hst, t in zip(host, d_dst):
                    t.copy_(hst)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            us = float(np.median(ts[3:])) * 1e6
            row = {"entry": "yardstick: download plus upload of the three planes, pageable host memory", "kind": "host clock around synchronous copies",
                   "width": w, "height": h, "bit_depth": bd, "us": round(us, 1), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}
            lines.append(row)
            print(json.dumps(row), flush=True)
    ctx.synchronize()
    ctx.close()


def resources(path):
    """the compiler's own resource remarks for csrc/fg_grain.hip"""
    src = os.path.join(ROOT, "svt-av1-1_amd", "csrc", "fg_grain.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                            os.path.join(tmp, "fg_grain.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    keep = ("Function Name", "TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy", "LDS Size", "Spill")
    with open(path, "w") as f:
        for ln in r.stderr.split("\n"):
            if "remark:" in ln and any(k in ln for k in keep):
                t = ln.split("remark:", 1)[1].split("[-Rpass")[0].rstrip()
                f.write(("Name:" + t.split("Function Name:")[1] if "Function Name" in t else "   " + t.strip()) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    lines = []
    if a.resources:
        return resources(a.resources)
    if a.cpu:
        cpu_yardstick(lines)
    else:
        device_times(lines, a.iters)
    if a.out:
        with open(a.out, "a") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
