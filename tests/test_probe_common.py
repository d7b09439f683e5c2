"""tools/probe_common.py: the resource-report filter, the row file, every migrated probe's --help (an import or path mistake in any of
them shows there), and on the GPU the stream, the two timers and the upload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
PROBES = ("inter_pred", "intra_pred", "warp", "dlf", "cfl", "lr", "lr_sgr", "lr_finish", "cdef", "film_grain", "pa_stats", "pa_noise", "pa_bitdepth",
          "ma_stats", "md_fast", "md_ifs", "md_full", "md_part", "inloop_me")


def _load():
    saved = list(sys.path)   # the module extends sys.path for the probes; the suite keeps its own
    sys.path.insert(0, TOOLS)
    try:
        import probe_common
    finally:
        sys.path[:] = saved
    return probe_common


pc = _load()

TAG = "[-Rpass-analysis=kernel-resource-usage]"
STDERR = "\n".join([
    f"csrc/x.hip:10:1: remark: Function Name: _ZN6svthip8a_kernelEPKhj {TAG}",
    f"csrc/x.hip:10:1: remark:     TotalSGPRs: 22 {TAG}",
    f"csrc/x.hip:10:1: remark:     VGPRs: 16 {TAG}",
    f"csrc/x.hip:10:1: remark:     AGPRs: 0 {TAG}",
    f"csrc/x.hip:10:1: remark:     ScratchSize [bytes/lane]: 0 {TAG}",
    f"csrc/x.hip:10:1: remark:     Dynamic Stack: False {TAG}",
    f"csrc/x.hip:10:1: remark:     Occupancy [waves/SIMD]: 8 {TAG}",
    f"csrc/x.hip:10:1: remark:     SGPRs Spill: 0 {TAG}",
    f"csrc/x.hip:10:1: remark:     VGPRs Spill: 3 {TAG}",
    f"csrc/x.hip:10:1: remark:     LDS Size [bytes/block]: 4096 {TAG}",
    "csrc/x.hip:31:9: warning: unused variable 'VGPRs' [-Wunused-variable]",
    f"csrc/x.hip:40:1: remark: Function Name: _ZN6svthip8b_kernelEPj {TAG}",
    f"csrc/x.hip:40:1: remark:     TotalSGPRs: 90 {TAG}",
    f"csrc/x.hip:40:1: remark:     VGPRs: 54 {TAG}",
    f"csrc/x.hip:40:1: remark:     AGPRs: 0 {TAG}",
    f"csrc/x.hip:40:1: remark:     ScratchSize [bytes/lane]: 16 {TAG}",
    f"csrc/x.hip:40:1: remark:     Occupancy [waves/SIMD]: 4 {TAG}",
    f"csrc/x.hip:40:1: remark:     SGPRs Spill: 2 {TAG}",
    f"csrc/x.hip:40:1: remark:     VGPRs Spill: 0 {TAG}",
    f"csrc/x.hip:40:1: remark:     LDS Size [bytes/block]: 0 {TAG}",
    "1 warning generated when compiling for gfx950.",
    ""])

WITH_SPILL = """Name: _ZN6svthip8a_kernelEPKhj
   TotalSGPRs: 22
   VGPRs: 16
   AGPRs: 0
   ScratchSize [bytes/lane]: 0
   Occupancy [waves/SIMD]: 8
   SGPRs Spill: 0
   VGPRs Spill: 3
   LDS Size [bytes/block]: 4096
Name: _ZN6svthip8b_kernelEPj
   TotalSGPRs: 90
   VGPRs: 54
   AGPRs: 0
   ScratchSize [bytes/lane]: 16
   Occupancy [waves/SIMD]: 4
   SGPRs Spill: 2
   VGPRs Spill: 0
   LDS Size [bytes/block]: 0
"""


def test_resource_report_filter():
    assert pc.resource_report(STDERR, spill=True) == WITH_SPILL
    # without "Spill" in the keep-list the SGPR spill lines go; "VGPRs Spill" stays, since "VGPRs" matches it (the committed reports have it so)
    without = "".join(ln + "\n" for ln in WITH_SPILL.splitlines() if "SGPRs Spill" not in ln)
    assert pc.resource_report(STDERR) == pc.resource_report(STDERR, spill=False) == without
    assert "Dynamic Stack" not in WITH_SPILL and "warning" not in pc.resource_report(STDERR, spill=True)


def test_write_rows(tmp_path):
    path = tmp_path / "rows.jsonl"
    first = [{"entry": "a", "us": 1.5, "ok": True}, {"entry": "b", "area": [64, 64], "copy_us": None}]
    second = [{"entry": "c", "kind": "host clock", "us": 20.0}]
    pc.write_rows(str(path), first, append=False)
    pc.write_rows(str(path), second)                       # append is the default
    assert [json.loads(ln) for ln in path.read_text().splitlines()] == first + second
    pc.write_rows(str(path), second, append=False)
    assert [json.loads(ln) for ln in path.read_text().splitlines()] == second
    pc.write_rows(None, first)                             # no --out: nothing is written
    assert [json.loads(ln) for ln in path.read_text().splitlines()] == second


def test_emit(capsys):
    lines = []
    pc.emit(lines, {"entry": "a", "us": 1.5})
    assert lines == [{"entry": "a", "us": 1.5}] and capsys.readouterr().out == '{"entry": "a", "us": 1.5}\n'


@pytest.mark.parametrize("probe", PROBES)
def test_probe_help(probe):
    r = subprocess.run([sys.executable, os.path.join(TOOLS, probe + "_probe.py"), "--help"], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--iters" in r.stdout and "--out" in r.stdout


@pytest.mark.gpu
def test_stream_timers_and_upload():
    import torch
    before = torch.cuda.current_stream()
    try:
        torch_stream, handle = pc.open_stream(torch)
        assert handle and handle == torch_stream.cuda_stream and torch.cuda.current_stream() == torch_stream
        x = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
        t = pc.timed(torch, lambda: x.add_(1), iters=3, reps=2)
        assert 0 < t.min <= t.median <= t.max, t
        torch_stream.synchronize()
        assert int(x[0]) == (3 + 3 * 2) % 256               # three warm calls, then three samples of two
        host = torch.zeros(1 << 20, dtype=torch.uint8)
        h = pc.host_timed(lambda: (host.copy_(x), torch_stream.synchronize()), 3, torch_stream.synchronize)
        assert 0 < h.min <= h.median <= h.max, h
        a = np.zeros(7, np.dtype([("offset", "<u4"), ("mv", "<i2", (2,)), ("flag", "u1")]))
        a["offset"], a["mv"], a["flag"] = np.arange(7) * 0x01020304, np.arange(14).reshape(7, 2) - 5, np.arange(7) + 240
        d = pc.as_dev(torch, a[::2])                        # not contiguous: the upload packs it
        assert d.dtype == torch.uint8 and d.is_cuda and d.cpu().numpy().tobytes() == np.ascontiguousarray(a[::2]).tobytes()
    finally:
        torch.cuda.set_stream(before)
