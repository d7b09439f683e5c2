"""CPU: the restatement of mode decision's full loop for the 128-wide blocks (tests/md_full128_util.py) against tests/golden/md_full128.npz
-- what the reference's own ProductFullLoop, FullLoop_R, CuFullDistortionFastTuMode_R, full cost and AV1PerformInverseTransformRecon returned
for the constructed blocks, and the recorded end-to-end results of the constructed cases -- and, where the reference is present, against
the live driver (tests/golden/ref_md_full128_driver.c).  Then the surface: the library exports the two entries, the header compiles as
C99 and the binding's layout of svthip_md_full128_tu is the header's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import md_full128_util as wu  # noqa: E402
import md_full_util as fu  # noqa: E402
import svtav1_hip  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


@pytest.mark.parametrize("name", list(wu.CASES))
def test_cases_equal_the_fixture(name):
    """the restated call equals the recorded rows, per-TU numbers, digests and refused count (expected() asserts them), and every slot
    with a cost equals what the reference returned for its candidate"""
    s, st, fx = wu.scenario(name), wu.expected(name), wu.fixture()
    assert len(st["result"]) == len(st["tu"]) == s.n_groups * s.max_full
    n_tu = int(fx[f"{name}__geometry"][0])
    assert n_tu == len(s.origins) and [tuple(o) for o in fx[f"{name}__geometry"][1:1 + 2 * n_tu].reshape(-1, 2).tolist()] == s.origins
    assert tuple(fx[f"{name}__geometry"][9:11]) == (wu.TS_Y, wu.TS_UV)
    slots = fx[f"{name}__ref_slots"].tolist()
    assert slots == [k for k in range(s.n_slots) if int(st["result"][k]["full_cost"]) != wu.U64] and slots
    for i, k in enumerate(slots):
        out64, out32, tiles = wu.restated_slot(s, st, k)
        assert np.array_equal(out64, fx[f"{name}__ref64"][i]) and np.array_equal(out32, fx[f"{name}__ref32"][i]), (name, k)
        assert fu.digest(tiles) == str(fx[f"{name}__ref_recon"][i]), (name, k, "the reconstruction is not the reference's")


def test_cases_hold_what_the_issue_asks_of_them():
    covered = {}
    for name in wu.CASES:
        cov = wu.coverage(wu.scenario(name), wu.expected(name))
        assert cov["y mask partial"], name
        for k, v in cov.items():
            covered[k] = covered.get(k, False) or v
    assert all(covered.values()), covered
    assert [(wu.scenario(n).n_groups, wu.scenario(n).max_full) for n in ("128x128", "128x64", "64x128")] == [(3, 3), (2, 1), (5, 12)]
    assert wu.expected("64x128")["refused"] >= 1 and any(int(d["n_full"]) == 0 for d in wu.expected("64x128")["decision"])


@pytest.mark.skipif(not reference_available(), reason="the reference is not on this machine")
def test_restatement_equals_the_live_reference(tmp_path):
    L = wu.build_reference_driver(str(tmp_path))
    for name in wu.CASES:
        s, st = wu.scenario(name), wu.expected(name)
        n_tu, org, ts_y, ts_uv = wu.reference_geometry(L, s.w, s.h)
        assert (n_tu, org, ts_y, ts_uv) == (len(s.origins), s.origins, wu.TS_Y, wu.TS_UV)
        for k in range(s.n_slots):
            if int(st["result"][k]["full_cost"]) == wu.U64:
                continue
            ref64, ref32, recon = wu.reference_slot(L, s, st["slots"][k]["row"])
            out64, out32, tiles = wu.restated_slot(s, st, k)
            assert np.array_equal(ref64, out64) and np.array_equal(ref32, out32), (name, k, ref64, out64, ref32, out32)
            assert all(np.array_equal(a, b) for a, b in zip(recon, tiles)), (name, k)


def test_surface(tmp_path):
    lib = svtav1_hip.lib()
    for symbol in ("svthip_md_full128_workspace_bytes", "svthip_md_full_loop128_batch_dev"):
        assert hasattr(lib, symbol), symbol
    assert callable(svtav1_hip.Context.md_full_loop128_batch_dev) and callable(svtav1_hip.md_full128_workspace_bytes)
    dt = svtav1_hip.md_full128_tu_dtype()
    assert dt.itemsize == 32 and dt.fields["eob"][0].shape == (3, 4) and dt.fields["eob"][0].base == np.dtype("<u2") and dt.fields["eob"][1] == 0
    c = tmp_path / "md_full128_header.c"
    c.write_text('#include <stddef.h>\n#include "svtav1_hip.h"\n'
                 f"typedef char size_is[sizeof(svthip_md_full128_tu) == {dt.itemsize} ? 1 : -1];\n"
                 f"typedef char eob_at[offsetof(svthip_md_full128_tu, eob) == {dt.fields['eob'][1]} ? 1 : -1];\n"
                 "typedef char eob_is[sizeof(((svthip_md_full128_tu *)0)->eob) == 3 * 4 * sizeof(uint16_t) ? 1 : -1];\n"
                 "size_t (*const bytes)(uint32_t, uint32_t, uint32_t, uint32_t) = svthip_md_full128_workspace_bytes;\n"
                 "int main(void) { return bytes(0, 0, 0, 0) != 0 || svthip_md_full_loop128_batch_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, "
                 "0, 0, 0, 0, 0) == 0; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:2000]
    # refused arguments need no device: 0 bytes for everything but the three sizes
    assert [svtav1_hip.md_full128_workspace_bytes(2, 3, w, h) > 0 for w, h in ((128, 128), (128, 64), (64, 128), (64, 64), (128, 32), (0, 0))] == \
        [True, True, True, False, False, False]
    assert svtav1_hip.md_full_workspace_bytes(2, 3, 128, 128, 1, 1) == 0   # the other entry still refuses them
    assert C.sizeof(svtav1_hip._abi.structure("svthip_md_full128_tu")) == 32
