"""What the timing probes under tools/ share: the import path, the private stream, the upload of a numpy array, the two ways of
measuring (device events behind a sleep kernel, the host clock around synchronous work), the JSON rows and their file, the compiler's
resource remarks, and the options every probe takes.  Plain functions: each probe keeps its own workload, its own check of what it timed
and its own rows.

Importing the module puts tests/, tests/golden/, tools/, the Python package and the repository root on sys.path."""
import collections
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "svt-av1-1_amd", "python"), ROOT]

Timing = collections.namedtuple("Timing", "median min max")   # microseconds, over the samples of one measurement


def open_stream(torch):
    """(torch stream, its handle): a stream of the probe's own, made current.  The default stream's handle is NULL, which the library reads
    as "the context's stream" -- events recorded on torch's current stream would then bracket nothing."""
    torch_stream = torch.cuda.Stream()
    torch.cuda.set_stream(torch_stream)
    assert torch_stream.cuda_stream
    return torch_stream, torch_stream.cuda_stream


def as_dev(torch, a):
    """the bytes of a numpy array (structured ones included) as a flat uint8 tensor on the device"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def timed(torch, fn, iters, reps=10):
    """device time of one fn() in microseconds, as a Timing over iters samples, each the mean of reps back-to-back calls: the current
    stream is held by a sleep kernel while the calls are queued behind it, so the events bracket the device's back-to-back execution and
    not the host's launch rate, which is slower than small calls (about 35 us for eleven launches from Python, whatever their size)"""
    s = torch.cuda.current_stream()
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(20_000_000)
        a.record(s)
        for _ in range(reps):
            fn()
        b.record(s)
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0 / reps)
    return Timing(float(np.median(ts)), float(min(ts)), float(max(ts)))


def host_timed(fn, iters, sync):
    """host-clock time of one fn() in microseconds, as a Timing over iters rounds after three warm ones; sync() runs before each round,
    outside the clock, and fn ends with whatever synchronise belongs to what it measures"""
    ts = []
    for _ in range(3 + iters):
        sync()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts = ts[3:]
    return Timing(float(np.median(ts)), float(min(ts)), float(max(ts)))


def emit(lines, row):
    lines.append(row)
    print(json.dumps(row), flush=True)


def write_rows(path, lines, append=True):
    """one JSON line per row to path, if one was given"""
    if path:
        with open(path, "a" if append else "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


def resource_report(stderr, spill=False):
    """the report text from the compiler's kernel-resource-usage remarks: a Name line per kernel, its figures indented below.  The keep-list
    matches by substring, so "VGPRs" keeps the "VGPRs Spill" line with or without spill; the committed reports have it that way."""
    keep = ("Function Name", "TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy", "LDS Size") + (("Spill",) if spill else ())
    out = []
    for ln in stderr.split("\n"):
        if "remark:" in ln and any(k in ln for k in keep):
            t = ln.split("remark:", 1)[1].split("[-Rpass")[0].rstrip()
            out.append(("Name:" + t.split("Function Name:")[1] if "Function Name" in t else "   " + t.strip()) + "\n")
    return "".join(out)


def resources(source, path, spill=False):
    """registers, scratch, LDS and occupancy of the kernels of csrc/<source>, from the compiler's own remarks, written to path"""
    src = os.path.join(ROOT, "svt-av1-1_amd", "csrc", source)
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                            os.path.join(tmp, os.path.splitext(source)[0] + ".o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(path, "w") as f:
        f.write(resource_report(r.stderr, spill))


def add_common_args(ap, iters_default, out_default=None, cpu=False, resources=False, tag=False):
    """--iters and --out, and of --cpu, --resources and --tag those the probe has"""
    ap.add_argument("--iters", type=int, default=iters_default)
    ap.add_argument("--out", default=out_default)
    if cpu:
        ap.add_argument("--cpu", action="store_true")
    if resources:
        ap.add_argument("--resources", default=None)
    if tag:
        ap.add_argument("--tag", default=None, help="a word kept in every row, e.g. which build was timed")
