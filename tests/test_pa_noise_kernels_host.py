"""CPU: the __device__ filter, noise, leaf, pyramid, flag and class arithmetic and the SB staging of svt-av1-1_amd/csrc/pa_noise_kernels.h
compiled for the host (tests/host_kernels/pa_noise_host.cpp behind tests/host_kernels/hip_on_host.h) and run over the 64x64 and 136x72
pictures of the reference's fixture (tests/golden/pa_noise.npz), both precisions; the pictures take all three arms of the denoise entry.  A
stand-alone program with its own main, built with -fsanitize=address,undefined; its luma plane has no border at all and its chroma planes
are exactly w/2 x h/2, so a read outside the interior ends the run.  What this cannot show -- the lane mapping, LDS, the barriers, the
device's byte-align instruction -- is what tests/test_pa_noise_gpu.py is for."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import pa_noise_util as nu  # noqa: E402
from lr_host_util import build_host_program  # noqa: E402

OUTPUTS = ("sb_var", "flat_noise", "picture", "denoised", "out_luma", "out_cb", "out_cr")


@pytest.fixture(scope="module")
def host_kernels(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pa_noise_host")
    return build_host_program(tmp, "pa_noise_host"), str(tmp)


@pytest.mark.parametrize("c", (0, 1))   # 64x64, 136x72
def test_device_arithmetic_matches_fixture_on_the_host(host_kernels, c):
    exe, tmp = host_kernels
    w, h, pics = nu.fixture_cases()[c]
    assert (w, h) == ((64, 64), (136, 72))[c]
    arms = set()
    for i, (luma, cb, cr, outs) in enumerate(pics):
        for sub in (0, 1):
            fin, fout = os.path.join(tmp, f"c{c}p{i}s{sub}_in.bin"), os.path.join(tmp, f"c{c}p{i}s{sub}_out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([w, h, sub], np.int32).tobytes() + b"".join(np.ascontiguousarray(p).tobytes() for p in (luma, cb, cr)))
            r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
            assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
            raw, at = open(fout, "rb").read(), 0
            for k in OUTPUTS:
                want = outs[sub][k]
                got = np.frombuffer(raw, want.dtype, want.size, at).reshape(want.shape)
                at += got.nbytes
                assert np.array_equal(got, want), ((w, h), i, sub, k)
            assert at == len(raw)
            arms.add(nu.arm(outs[sub]["picture"]))
    assert arms == set(nu.ARMS)
