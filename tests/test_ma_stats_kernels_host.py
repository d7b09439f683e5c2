"""CPU: the __device__ arithmetic of svt-av1-1_amd/csrc/ma_stats_kernels.h compiled for the host (tests/host_kernels/ma_stats_host.cpp behind
tests/host_kernels/hip_on_host.h) and run over the 64x64 and 136x72 items of the reference's fixture (tests/golden/ma_stats.npz).  A stand-alone
program with its own main, built with -fsanitize=address,undefined; its planes carry exactly the border the entries require and its tables
exactly their entries, so a read outside them ends the run.  What this cannot show -- the lane mapping, the wave reductions, the LDS counters
and the device's packed byte instruction -- is what tests/test_ma_stats_gpu.py is for."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import ma_stats_util as mu  # noqa: E402
from lr_host_util import build_host_program  # noqa: E402


@pytest.fixture(scope="module")
def host_kernels(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ma_stats_host")
    return build_host_program(tmp, "ma_stats_host"), str(tmp)


def _run(host_kernels, mode, name, header, arrays, wanted):
    """wanted: [(dtype, shape)] -> the arrays the program wrote"""
    exe, tmp = host_kernels
    fin, fout = os.path.join(tmp, name + "_in.bin"), os.path.join(tmp, name + "_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array(header, np.int32).tobytes() + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))
    r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, out = open(fout, "rb").read(), 0, []
    for dt, shape in wanted:
        out.append(np.frombuffer(raw, dt, int(np.prod(shape)), at).reshape(shape))
        at += out[-1].nbytes
    assert at == len(raw)
    return out


@pytest.mark.parametrize("c", (0, 1))   # 64x64, 136x72
def test_device_arithmetic_matches_fixture_on_the_host(host_kernels, c):
    w, h, groups = mu.fixture_cases()[c]
    assert (w, h) == ((64, 64), (136, 72))[c]
    n = mu.n_sbs(w, h)
    for i, item in enumerate(groups["zz"]):
        got = _run(host_kernels, "zz", f"c{c}zz{i}", [w, h], [item["cur"], item["prev"]], [(np.uint32, (n,)), (np.uint8, (n,)), (np.uint8, (n,))])
        for k, g in zip(mu.ZZ_KEYS[2:], got):
            assert np.array_equal(g, item[k]), ((w, h), "zz", i, k)
    for i, item in enumerate(groups["energy"]):
        got = _run(host_kernels, "energy", f"c{c}en{i}", [w, h, int(item["intra"])], [item["luma"], item["y_mean"]], [(np.uint64, (n, 5))] * 2)
        for k, g in zip(mu.ENERGY_KEYS[3:], got):
            assert np.array_equal(g, item[k]), ((w, h), "energy", i, k)
    for i, item in enumerate(groups["tables"]):
        mine = mu.all_tables(item, w, h)
        got = _run(host_kernels, "tables", f"c{c}tb{i}", [w, h] + [int(v) for v in item["signals"]],
                   [item["me"], item["cand"], item["y_mean"], item["variance"], item["ref_mean"], item["ref_var"]],
                   [(np.uint32, (n,))] * 3 + [(np.uint32, (2, 128)), (np.uint32, ()), (np.int32, (12,)), (np.uint8, (n, 4))])
        for k, g in zip(("rc_me_distortion", "inter_index", "intra_index", "histograms", "full_sb_count", "global_motion", "flags"), got):
            assert np.array_equal(g, mine[k]), ((w, h), "tables", i, k, g, mine[k])
        assert np.array_equal(got[6], item["flags"])
        if item["compare_global_motion"]:
            assert np.array_equal(got[5][:6], item["global_motion"])
