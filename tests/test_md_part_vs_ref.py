"""CPU: the restatement of mode decision's partition decision (tests/md_part_util.py) against tests/golden/md_part.npz -- what the reference's
own d1_non_square_block_decision, d2_inter_depth_block_decision and EncodePass's walk gave for the cases -- and, where the reference is
present, against the live driver (tests/golden/ref_md_part_driver.c); and the block table of the library (svthip_md_partition_geometry)
against the restated recursion and the reference's blk_geom_mds."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import md_part_util as pu  # noqa: E402
import svtav1_hip  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


@pytest.mark.parametrize("name", pu.CASES)
def test_restatement_equals_the_fixture(name):
    s, e, fx = pu.scenario(name), pu.expected(name), pu.fixture()
    assert [pu.state_digest(r) for r in e["walks"]] == fx[f"{name}__state"].tolist()
    assert np.array_equal(e["count"], fx[f"{name}__count"])
    assert [m for r in e["walks"] for m in r["final"]] == fx[f"{name}__final"].tolist()
    assert e["count"].max() <= (1024 if s.sb_size == 128 else 256)


def test_cases_hold_what_the_issue_asks_of_them():
    stats = pu.assert_coverage(pu.CASES)
    assert stats["stale_root"] >= 1 and stats["d1_ties"] >= 1 and stats["d2_ties"] >= 1
    arms = pu.fixture()["split_flag_rate_arms"].tolist()
    assert arms[0] > 0 and arms[0] == arms[1] and arms[2] == 0   # every Av1SplitFlagRate call took the hasRows && hasCols arm
    # the irregular list: the climb of the last 32x32 saw the cost the H shape left, the square ends with the V shape's
    s, e = pu.scenario("p64-irregular-p-v0"), pu.expected("p64-irregular-p-v0")
    r, q3 = e["walks"][0], 25 + 3 * 269
    assert r["cost"][q3] == 18000 and r["part"][q3] == 2 and r["part"][0] == pu.SPLIT
    others = sum(r["cost"][25 + k * 269] for k in range(3))
    assert r["cost"][0] == others + 60000 + pu.rate(s.fac, s.lams[0], 64, 1) + 4 * pu.rate(s.fac, s.lams[0], 32, 0)
    assert pu.expected("p64-leafless-p-v0")["refused"] == 1 and int(pu.expected("p64-leafless-p-v0")["final"][0][0]["leaf"]) == pu.NONE
    # a cost of ~0 sits in a listed shape of the ties cases
    assert any(c == pu.M64 for c in pu.scenario("p64-all-p-ties").costs[0])


@pytest.mark.parametrize("sb_size", (64, 128))
def test_library_geometry_is_the_restated_recursion(sb_size):
    ours, want = svtav1_hip.md_partition_geometry(sb_size), pu.geometry(sb_size)
    assert ours.dtype == svtav1_hip.md_partition_block_dtype() and ours.dtype.itemsize == 16
    assert len(ours) == len(want) == {64: 1101, 128: 4421}[sb_size] and int((ours["shape"] == 0).sum()) == {64: 341, 128: 1365}[sb_size]
    for field in want.dtype.names:
        assert np.array_equal(ours[field], want[field]), field
    # the distances to the parent square of a last quadrant: 8 / 52 / 208 / 832 / 3320
    last = ours[(ours["shape"] == 0) & (ours["is_last_quadrant"] == 1)]
    dist = {int(sb_size >> b["depth"]): int(b["sqi_mds"]) - int(b["parent_mds"]) for b in last}
    assert dist == {k: v for k, v in {4: 8, 8: 52, 16: 208, 32: 832, 64: 3320}.items() if k < sb_size}


@pytest.mark.skipif(not reference_available(), reason="the reference is not on this machine")
def test_restatement_and_geometry_equal_the_live_reference(tmp_path):
    L = pu.build_reference_driver(str(tmp_path))
    for sb_size in (64, 128):
        ref, ours = pu.reference_geometry(L, sb_size), svtav1_hip.md_partition_geometry(sb_size)
        for i, field in enumerate(pu.REF_GEOM_FIELDS):
            assert np.array_equal(ref[:, i], ours[field].astype(np.int32)), (sb_size, field)
    for name in pu.CASES:
        s, e = pu.scenario(name), pu.expected(name)
        for k in range(len(s.origins)):
            r, counters = pu.reference_walk(L, s, k)
            for key in ("cost", "part", "split", "best", "tested", "mdc", "final"):
                assert r[key] == e["walks"][k][key], (name, k, key)
            assert counters[1] == counters[2] and counters[3] == 0, (name, k, counters)
