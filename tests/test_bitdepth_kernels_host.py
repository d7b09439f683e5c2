"""CPU: the lane functions of svt-av1-1_amd/csrc/pa_bitdepth_kernels.h -- the unpack / pack / compressed-pack sample arithmetic, the head, whole
piece and tail split of every row, the offsets into the SB-tiled compressed plane, the block -> plane -> row -> piece map of the flat grid --
compiled for the host (tests/host_kernels/pa_bitdepth_host.cpp behind tests/host_kernels/hip_on_host.h) and run over every picture of both
fixture sizes (tests/golden/bitdepth.npz), the maximal-difference pictures included.  A stand-alone program with its own main, built with
-fsanitize=address,undefined; every plane is an allocation of exactly its interior, so an access outside an interior ends the run.  What
this cannot show -- the wave and workgroup reductions, the finish kernel, the device's 16-byte accesses at odd addresses -- is what
tests/test_bitdepth_gpu.py is for."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import bitdepth_util as bu  # noqa: E402
from lr_host_util import build_host_program  # noqa: E402


@pytest.fixture(scope="module")
def host_kernels(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pa_bitdepth_host")
    return build_host_program(tmp, "pa_bitdepth_host"), str(tmp)


def run(exe, tmp, tag, w, h, in16, inn, tiled, recon8, recon16):
    fin, fout = os.path.join(tmp, tag + "_in.bin"), os.path.join(tmp, tag + "_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([w, h], np.int32).tobytes())
        for c in range(3):
            f.write(b"".join(np.ascontiguousarray(a[c]).tobytes() for a in (in16, inn, tiled, recon8, recon16)))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, got = open(fout, "rb").read(), 0, {}
    for c, (ph, pw) in enumerate(bu.plane_dims(w, h)):
        for k, dt in (("out8", np.uint8), ("outn", np.uint8), ("out8_alone", np.uint8), ("pack16", np.uint16), ("packc16", np.uint16)):
            a = np.frombuffer(raw, dt, ph * pw, at).reshape(ph, pw)
            at += a.nbytes
            got.setdefault(k, []).append(a)
    for k in ("sse8", "sse16", "sse16_unpacked", "sse16_compressed"):
        got[k] = np.frombuffer(raw, np.uint64, 3, at)
        at += 24
    assert at == len(raw)
    return got


@pytest.mark.parametrize("c", (0, 1))   # 72x40, 136x72
def test_lane_functions_match_fixture_on_the_host(host_kernels, c):
    exe, tmp = host_kernels
    w, h, pics = bu.fixture_pictures(c)
    assert (w, h) == bu.CASES[c]
    for i, p in enumerate(pics):
        got = run(exe, tmp, f"c{c}p{i}", w, h, p["in16"], p["inn"], p["tiled"], p["recon8"], p["recon16"])
        for k in ("out8", "outn", "pack16", "packc16"):
            for pl in range(3):
                assert np.array_equal(got[k][pl], p[k][pl]), ((w, h), i, k, bu.PLANES[pl])
        assert all(np.array_equal(a, b) for a, b in zip(got["out8_alone"], p["out8"]))
        for k in ("sse8", "sse16_unpacked", "sse16_compressed"):
            assert np.array_equal(bu.reference_fields(got[k]), p[k]), ((w, h), i, k)
        assert np.array_equal(got["sse16"], got["sse16_unpacked"])
        assert np.array_equal(got["sse16_unpacked"], bu.picture_sse(p["recon16"], p["pack16"]))


@pytest.mark.parametrize("c", (0, 1))
def test_maximal_differences_keep_64_bits_on_the_host(host_kernels, c):
    exe, tmp = host_kernels
    w, h, p = bu.fixture_max_difference(c)
    in16 = [a.astype(np.uint16) << 2 for a in p["in8"]]
    got = run(exe, tmp, f"c{c}max", w, h, in16, p["inn"], p["tiled"], p["recon8"], p["recon16"])
    want = bu.expected_max_difference(p)
    for k in want:
        assert np.array_equal(got[k], want[k]), ((w, h), k)
        assert np.array_equal(bu.reference_fields(got[k]), p[k]), ((w, h), k)
    if c == 1:
        assert int(want["sse16_unpacked"][0]) >= 1 << 32
