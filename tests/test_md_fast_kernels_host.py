"""CPU: the __device__ arithmetic of svt-av1-1_amd/csrc/md_fast_kernels.h -- the quad walk of a candidate's lanes over Y, Cb and Cr, the flags,
the cost, the buffer walk and PreModeDecision -- compiled for the host (tests/host_kernels/md_fast_host.cpp behind
tests/host_kernels/hip_on_host.h) and run for every one of the 22 sizes.  A stand-alone program with its own main, built with
-fsanitize=address,undefined.  Its planes are allocated to exactly their size: the source picture's last block lies in its last rows and
columns, and the pool planes are cut where the last tile ends, so a read beyond a block ends the run.  Each size runs with the planes 0, 1,
2 and 3 bytes into their allocations (the dword and the byte path).  What this cannot show -- the sum over the lanes, the LDS columns of the
pick, the vector loads and stores -- is what tests/test_md_fast_gpu.py is for."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import md_fast_util as mu  # noqa: E402
from lr_host_util import build_host_program  # noqa: E402

N_DESC = 13


@pytest.fixture(scope="module")
def host_kernels(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("md_fast_host")
    return build_host_program(tmp, "md_fast_host"), str(tmp)


def cut_pool(z, pool):
    """the pool planes cut right behind the last tile: its last sample is the last of each plane"""
    w, h = mu.SIZES[z]
    cw, ch = mu.chroma_size(w, h)
    x, y = mu.tile_origins(w, h)[0][-1]
    cx, cy = mu.round_uv(x), mu.round_uv(y)
    return [np.ascontiguousarray(pool[0][:y + h, :x + w]), np.ascontiguousarray(pool[1][:cy + ch, :cx + cw]), np.ascontiguousarray(pool[2][:cy + ch, :cx + cw])]


@pytest.mark.parametrize("z", range(len(mu.SIZES)))
def test_device_arithmetic_matches_reference_on_the_host(host_kernels, z):
    exe, tmp = host_kernels
    w, h = mu.SIZES[z]
    fx = mu.fixture()
    src = mu.source_planes()
    pool = cut_pool(z, mu.pool_planes(z, src))
    desc = mu.descriptors(z, N_DESC)
    assert (int(desc[5]["src_x"]) + w, int(desc[5]["src_y"]) + h) == (mu.SRC_W, mu.SRC_H)
    assert (int(desc[5]["pred_x"]) + w, int(desc[5]["pred_y"]) + h) == pool[0].shape[::-1]
    p_result, p_desc, groups = mu.pick_inputs()
    bad = np.array([(0, 0, 3, 13), (0, 114, 3, 13), (0, 3, 3, 0), (0, 3, 3, 14), (0, 3, 0, 13), (0, 3, 13, 13), (len(p_result) - 2, 3, 3, 13)], mu.GROUP_DTYPE)
    groups = np.concatenate([groups, bad])
    want = mu.fast_cost(src, pool, desc, w, h)
    assert np.array_equal(want, np.ascontiguousarray(fx[f"result_z{z}"]).view(mu.RESULT_DTYPE).reshape(-1)), "differs from the reference"
    want_pick, want_refused = mu.pick(p_result, p_desc, groups)
    assert np.array_equal(want_pick[:len(fx["pick"])].view(np.uint8).reshape(-1, 32), fx["pick"]), "differs from the reference"
    for shift in range(4):
        fin, fout = os.path.join(tmp, f"z{z}s{shift}_in.bin"), os.path.join(tmp, f"z{z}s{shift}_out.bin")
        head = [w, h, len(desc), mu.SRC_W, mu.SRC_H, mu.SRC_W // 2, mu.SRC_H // 2, pool[0].shape[1], pool[0].shape[0], pool[1].shape[1], pool[1].shape[0],
                shift, len(p_result), len(groups)]
        with open(fin, "wb") as f:
            f.write(np.array(head, np.int32).tobytes() + b"".join(np.ascontiguousarray(a).tobytes() for a in (*src, *pool)) + desc.tobytes()
                    + p_result.tobytes() + p_desc.tobytes() + groups.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        raw = open(fout, "rb").read()
        got = np.frombuffer(raw, mu.RESULT_DTYPE, len(desc))
        got_pick = np.frombuffer(raw, mu.PICK_DTYPE, len(groups), got.nbytes)
        assert len(raw) == got.nbytes + got_pick.nbytes + 4
        assert np.array_equal(got, want), ((w, h), shift, np.flatnonzero(got != want)[:6])
        assert np.array_equal(got_pick, want_pick), ((w, h), shift, np.flatnonzero(got_pick != want_pick)[:6])
        assert int(np.frombuffer(raw, np.int32, 1, got.nbytes + got_pick.nbytes)[0]) == want_refused == len(bad)
