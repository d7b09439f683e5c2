"""CPU: the __device__ arithmetic and the SB / region index geometry of svt-av1-1_amd/csrc/pa_stats_kernels.h compiled for the host
(tests/host_kernels/pa_stats_host.cpp behind tests/host_kernels/hip_on_host.h) and run over the 64x64 and 136x72 pictures of the reference's
fixture (tests/golden/pa_stats.npz), both precisions.  A stand-alone program with its own main, built with -fsanitize=address,undefined; its
planes carry exactly the border the entries require, so a read outside them ends the run.  What this cannot show -- the lane mapping, LDS,
the barriers, the device's packed byte instructions and unaligned row loads -- is what tests/test_pa_stats_gpu.py is for."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import pa_stats_util as pu  # noqa: E402
from lr_host_util import build_host_program  # noqa: E402

SHAPES = {"y_mean": (np.uint8, 85), "variance": (np.uint16, 85), "cb_mean": (np.uint8, 21), "cr_mean": (np.uint8, 21), "var_of_var": (np.uint64, 4),
          "homogeneous": (np.uint8, 1)}


@pytest.fixture(scope="module")
def host_kernels(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pa_stats_host")
    return build_host_program(tmp, "pa_stats_host"), str(tmp)


@pytest.mark.parametrize("c", (0, 1))   # 64x64, 136x72
def test_device_arithmetic_matches_fixture_on_the_host(host_kernels, c):
    exe, tmp = host_kernels
    w, h, pics = pu.fixture_cases()[c]
    assert (w, h) == ((64, 64), (136, 72))[c]
    n_sb = pu.sb_grid(w, h)[0] * pu.sb_grid(w, h)[1]
    for i, (luma, cb, cr, outs) in enumerate(pics):
        for sub in (0, 1):
            fin, fout = os.path.join(tmp, f"c{c}p{i}s{sub}_in.bin"), os.path.join(tmp, f"c{c}p{i}s{sub}_out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([w, h, sub], np.int32).tobytes() + b"".join(np.ascontiguousarray(p).tobytes() for p in (luma, cb, cr)))
            r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
            assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
            raw, at = open(fout, "rb").read(), 0
            for k in pu.OUTPUTS:
                want = outs[sub][k]
                got = np.frombuffer(raw, want.dtype, want.size, at).reshape(want.shape)
                at += got.nbytes
                if k in SHAPES:
                    assert want.dtype == SHAPES[k][0] and want.size == n_sb * SHAPES[k][1]
                assert np.array_equal(got, want), ((w, h), i, sub, k)
            assert at == len(raw)
