"""CPU: the Wiener kernels of svt-av1-1_amd/csrc/lr_wiener_kernels.h compiled for the host and run against the reference's fixture
(tests/golden/lr.npz), so that the device code's arithmetic, indexing and stripe rule are checked where there is no GPU.
tests/host_kernels/lr_wiener_host.cpp includes the kernel header behind tests/host_kernels/hip_on_host.h (one lane per workgroup, blockIdx /
threadIdx as globals, atomicAdd as a plain add) and runs every kernel over the grid function the launch code calls, so a wrong grid fails
here too.  A stand-alone program with its own main, built with -fsanitize=address,undefined: an index past an LDS array or a plane ends the
run.  What this cannot show -- lanes racing, the launch code's arguments -- is what tests/test_lr_gpu.py is for."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

from lr_host_util import build_host_program  # noqa: E402
from test_lr_vs_ref import fixture_case, unit_traces  # noqa: E402


@pytest.fixture(scope="module")
def host_kernels(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lr_host")
    return build_host_program(tmp, "lr_wiener_host"), str(tmp)


@pytest.mark.parametrize("c", (1, 2, 4, 6))
def test_kernel_bodies_match_fixture_on_the_host(host_kernels, c):
    """statistics, solve, the SSE of each unit's first recorded trial, and the frame filter of the mixed run (run 1)"""
    exe, tmp = host_kernels
    F = fixture_case(c)
    n = F["base"][3]
    traces = unit_traces(F)
    trial = np.array([traces[u][0][0] if traces[u] else F["start"][u] for u in range(n)], np.int16)
    fin, fout = os.path.join(tmp, f"in{c}.bin"), os.path.join(tmp, f"out{c}.bin")
    with open(fin, "wb") as f:
        f.write(np.array([F["w"], F["h"], F["bd"], *F["unit_size"], n, 0], np.int32).tobytes())
        for p in range(3):
            for k in ("cdef", "dbk", "src"):
                f.write(np.ascontiguousarray(F[k][p]).tobytes())
        f.write(trial.tobytes() + np.ascontiguousarray(F["utaps"][1]).tobytes() + np.ascontiguousarray(F["utype"][1]).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = open(fout, "rb").read()
    at = 0

    def take(dtype, shape):
        nonlocal at
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at).reshape(shape)
        at += a.nbytes
        return a

    M, H, none, avg = take(np.int64, (n, 49)), take(np.int64, (n, 2401)), take(np.int64, n), take(np.int32, n)
    rej, start, sse = take(np.int32, n), take(np.int16, (n, 16)), take(np.uint64, n)
    dt = np.uint16 if F["bd"] > 8 else np.uint8
    out = [take(dt, F["cdef"][p].shape) for p in range(3)]
    for u in range(n):
        k = F["win"][u] ** 2
        assert np.array_equal(M[u, :k], F["M"][u][:k]) and np.array_equal(H[u, :k * k], F["H"][u][:k * k]), (c, u)
        assert (M[u, k:] == -1).all() and (H[u, k * k:] == -1).all()
        if traces[u]:
            assert int(sse[u]) == traces[u][0][1], (c, u)
    assert np.array_equal(avg, F["avg"]) and np.array_equal(none, F["sse"][:, 0])
    assert np.array_equal(start, F["start"]) and np.array_equal(rej, F["rejected"])
    for p in range(3):
        assert np.array_equal(out[p], F["out"][1][p]), (c, p)
