"""CPU: the __device__ code of svt-av1-1_amd/csrc/md_part_kernels.h -- the geometry from the index, the decision of a superblock, the final
list and the composition -- compiled for the host (tests/host_kernels/md_part_host.cpp behind tests/host_kernels/hip_on_host.h) and run on
the fixture's cases of tests/md_part_util.py.  A stand-alone program with its own main, built with -fsanitize=address,undefined.  The pool
and the destination planes are allocated to exactly their size, so a copy beyond a plane ends the run, in four layouts that between them
take every arm of md_part_copy_tile:
    stride = width, 0 bytes into the allocation     units of 8 and 4 bytes at most (the widths are 136 / 68 and 264 / 132)
    stride = width, 2 and 3 bytes in                the 2-byte unit and single bytes
    stride a multiple of 16 whatever the width      the 16-byte unit, the one real pictures take; the columns between width and stride hold
                                                    a guard that must come back unchanged
The program reports in which unit it copied every tile; the test computes the same tally from the rule (the widest unit that both
addresses, both strides and the width are multiples of) and compares, so a layout that misses the arm it is here for fails.  All three
planes are compared in every layout.  Nothing loaded into Python runs under a sanitiser.  What this cannot show -- 256 lanes of a workgroup
together, the LDS, the barriers -- is what tests/test_md_part_gpu.py is for."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import md_part_util as pu  # noqa: E402
from lr_host_util import build_host_program  # noqa: E402

LAYOUTS = ((0, 0), (3, 0), (2, 0), (0, 1))   # (bytes into the allocation, stride a multiple of 16)
GUARD = 0x77


@pytest.fixture(scope="module")
def host_kernels(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("md_part_host")
    return build_host_program(tmp, "md_part_host"), str(tmp)


def _stride(width, pad):
    return (width + 15) // 16 * 16 + 16 if pad else width


def _padded(plane, pad):
    out = np.full((plane.shape[0], _stride(plane.shape[1], pad)), GUARD, np.uint8)
    out[:, :plane.shape[1]] = plane
    return out


def _unit(*values):
    bits = 16
    for v in values:
        bits |= v
    return bits & -bits


def _expected_units(s, e, shift, pad):
    """tiles per unit [1, 2, 4, 8, 16]: new[] gives 16-aligned memory, so an address is (shift + offset) modulo 16"""
    tally = [0] * 5
    ps, ds = (_stride(s.pool_w, pad), _stride(s.pool_w // 2, pad)), (_stride(s.w, pad), _stride((s.w + 1) // 2, pad))
    for k in range(len(s.origins)):
        for f in e["final"][k][:e["count"][k]]:
            if int(f["leaf"]) == pu.NONE:
                continue
            leaf = s.leaves[int(f["leaf"])]
            x, y, w, h, px, py = (int(v) for v in (f["x"], f["y"], f["bwidth"], f["bheight"], leaf["pool_x"], leaf["pool_y"]))
            tally[_unit(shift + y * ds[0] + x, shift + py * ps[0] + px, ds[0], ps[0], w).bit_length() - 1] += 1
            if f["has_uv"]:
                cx, cy, pcx, pcy = (((v >> 3) << 3) // 2 for v in (x, y, px, py))
                tally[_unit(shift + cy * ds[1] + cx, shift + pcy * ps[1] + pcx, ds[1], ps[1], max(4, w // 2)).bit_length() - 1] += 2
    return tally


@pytest.mark.parametrize("name", pu.CASES)
def test_device_code_matches_restatement_on_the_host(host_kernels, name):
    exe, tmp = host_kernels
    s, e = pu.scenario(name), pu.expected(name)
    g = pu.geometry(s.sb_size)
    n_sb, n, max_final = len(s.origins), len(g), e["final"].shape[1]
    dst0 = [np.full(p.shape, 0xA5, np.uint8) for p in e["dst"]]
    for shift, pad in LAYOUTS:
        head = [s.sb_size, int(s.intra), n_sb, len(s.leaves), len(s.decisions), shift, s.pool_w, s.pool_h, s.w, s.h, pad]
        fin, fout = os.path.join(tmp, f"{name}_{shift}_{pad}_in.bin"), os.path.join(tmp, f"{name}_{shift}_{pad}_out.bin")
        with open(fin, "wb") as f:
            f.write(np.array(head, np.int32).tobytes() + np.ascontiguousarray(s.fac, np.int32).tobytes()
                    + b"".join(a.tobytes() for a in (s.sbs, s.leaves, s.decisions))
                    + b"".join(_padded(p, pad).tobytes() for p in (*s.pool, *dst0)))
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        raw = open(fout, "rb").read()
        at = 0

        def take(dtype, count):
            nonlocal at
            a = np.frombuffer(raw, dtype, count, at)
            at += a.nbytes
            return a

        geom, result, final = take(pu.GEOM_DTYPE, n), take(pu.RESULT_DTYPE, n_sb * n).reshape(n_sb, n), take(pu.FINAL_DTYPE, n_sb * max_final).reshape(n_sb, max_final)
        count, refused, units = take(np.uint32, n_sb), int(take(np.int32, 1)[0]), take(np.uint32, 5).tolist()
        dst = [take(np.uint8, p.shape[0] * _stride(p.shape[1], pad)).reshape(p.shape[0], -1) for p in dst0]
        assert at == len(raw)
        assert np.array_equal(geom, g)
        assert np.array_equal(count, e["count"]) and refused == e["refused"]
        for k in range(n_sb):
            assert np.array_equal(result[k], e["result"][k]), (name, k, np.nonzero(result[k] != e["result"][k])[0][:5])
            assert np.array_equal(final[k][:count[k]], e["final"][k][:count[k]]), (name, k)
        for p, (a, b) in enumerate(zip(dst, e["dst"])):
            assert np.array_equal(a, _padded(b, pad)), (name, shift, pad, "composed plane or the columns behind it", p)
        assert units == _expected_units(s, e, shift, pad), (name, shift, pad, units)
        if shift == 3:
            assert units[1:] == [0, 0, 0, 0] and units[0] > 0
        if shift == 2:
            assert units[0] == 0 and units[2:] == [0, 0, 0] and units[1] > 0
        os.remove(fin), os.remove(fout)


def test_the_layouts_take_every_unit_on_all_three_planes():
    """over the cases, from the rule alone: the 16-byte unit is taken by luma AND chroma tiles in the padded layout, 8 and 4 in the plain one"""
    luma16 = chroma16 = plain8 = plain4 = 0
    for name in pu.CASES:
        s, e = pu.scenario(name), pu.expected(name)
        t = _expected_units(s, e, 0, 1)
        only_luma = [0] * 5
        ps, ds = _stride(s.pool_w, 1), _stride(s.w, 1)
        for k in range(len(s.origins)):
            for f in e["final"][k][:e["count"][k]]:
                if int(f["leaf"]) != pu.NONE:
                    leaf = s.leaves[int(f["leaf"])]
                    only_luma[_unit(int(f["y"]) * ds + int(f["x"]), int(leaf["pool_y"]) * ps + int(leaf["pool_x"]), int(f["bwidth"])).bit_length() - 1] += 1
        luma16, chroma16 = luma16 + only_luma[4], chroma16 + t[4] - only_luma[4]
        plain = _expected_units(s, e, 0, 0)
        plain8, plain4 = plain8 + plain[3], plain4 + plain[2]
        assert plain[4] == 0   # stride = width never reaches 16 bytes with these pictures: the padded layout is what does
    assert luma16 > 100 and chroma16 > 20 and plain8 > 100 and plain4 > 100, (luma16, chroma16, plain8, plain4)
