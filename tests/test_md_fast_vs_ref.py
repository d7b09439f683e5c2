"""CPU: the restatement of mode decision's fast loop (tests/md_fast_util.py) against the reference -- against the recorded fixture
(tests/golden/md_fast.npz) everywhere, and against the live driver (tests/golden/ref_md_fast_driver.c: the reference's SAD table in both asm
rows, its RDCOST macro, its PreModeDecision) where the reference is available.  The buffer walk of ProductPerformFastLoop is restated and
pinned by neither; its rules are checked here against hand-worked cases."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import md_fast_util as mu  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

N_DESC = 13


def _crcs(planes):
    return [zlib.crc32(np.ascontiguousarray(p).tobytes()) for p in planes]


def test_fixture_has_the_cases():
    z = mu.fixture()
    assert [tuple(int(v) for v in s) for s in z["sizes"]] == list(mu.SIZES) and len(set(mu.SIZES)) == 22
    assert os.path.getsize(mu.FIXTURE) <= 300_000
    assert list(z["src_crc"]) == _crcs(mu.source_planes())
    names = [c[0] for c in mu.pick_cases()]
    assert list(z["pick_names"]) == names and z["pick"].shape == (len(names), 32)
    assert sum(len(c[1]) == mu.MAX_CANDIDATES and c[4] == mu.MAX_BUFFERS for c in mu.pick_cases()) >= 2
    flags = {int(f) for f in mu.descriptors(0, N_DESC)["flags"]}
    assert flags == set(mu.flag_sets()) and all(any(f == bit for f in flags) for bit in (1, 2, 4, 8, 16))


@pytest.mark.parametrize("z", range(len(mu.SIZES)))
def test_fast_cost_matches_fixture(z):
    fx = mu.fixture()
    w, h = mu.SIZES[z]
    src = mu.source_planes()
    pool = mu.pool_planes(z, src)
    assert list(fx["pool_crc"][z]) == _crcs(pool)
    desc = mu.descriptors(z, N_DESC)
    for i, d in enumerate(desc):
        assert mu.candidate_sads(src, pool, d, w, h) == tuple(int(v) for v in fx[f"sads_z{z}"][i]), ((w, h), i)
    want = np.ascontiguousarray(fx[f"result_z{z}"]).view(mu.RESULT_DTYPE).reshape(-1)
    got = mu.fast_cost(src, pool, desc, w, h)
    assert np.array_equal(got, want), ((w, h), got, want)
    assert {0, 1} == {int(v) for v in desc["has_uv"]} and (want["cost"] == mu.MAX_COST).any() and (want["chroma"] > 0).any()


def test_pick_matches_fixture():
    fx = mu.fixture()
    result, desc, groups = mu.pick_inputs()
    got, refused = mu.pick(result, desc, groups)
    want = np.ascontiguousarray(fx["pick"]).view(mu.PICK_DTYPE).reshape(-1)
    assert refused == 0
    for name, g, w in zip(fx["pick_names"], got, want):
        assert g == w, (name, g, w)


def test_walk_by_hand():
    """the rules the walk and PreModeDecision turn on, worked by hand"""
    M = int(mu.MAX_COST)
    # three buffers: 50, 40 and 60 fill buffers 0, 1, 2; 30 replaces the 60 in buffer 2; the last candidate replaces the 50 in buffer 0
    assert mu.walk([50, 40, 60, 30, 70], 3) == ([70, 40, 30] + [M] * 10, [4, 1, 3] + [0xFF] * 10)
    # strict >: of two buffers at 90 the first is replaced
    assert mu.walk([90, 90, 10], 2)[1][:2] == [2, 1]
    # a cost of ~0 ends the search at once: the candidate in buffer 0 is replaced although buffer 1 is empty
    assert mu.walk([M, 40], 3)[1][:3] == [1, 0xFF, 0xFF]
    # the search is skipped after the last candidate and runs once even with one buffer
    assert mu.walk([50, 40], 1)[1][:2] == [0, 1]
    # PreModeDecision: >= leaves the LAST of two equal highest costs out; an intra entry moves behind a later inter entry
    assert mu.pre_mode_decision([80, 10, 80] + [M] * 10, [2, 1, 1] + [0] * 10, 3, False) == ([1, 0], 2, 1)
    assert mu.pre_mode_decision([5, 6, 7] + [M] * 10, [2, 2, 2] + [0] * 10, 3, True) == ([0, 1, 2], 3, 0)


def test_refused_groups():
    result, desc, _ = mu.pick_inputs()
    bad = np.array([(0, 0, 3, 13), (0, 114, 3, 13), (0, 3, 3, 0), (0, 3, 3, 14), (0, 3, 0, 13), (0, 3, 13, 13), (len(result) - 2, 3, 3, 13)], mu.GROUP_DTYPE)
    got, refused = mu.pick(result, desc, bad)
    assert refused == len(bad) and (got["best"] == 0xFF).all() and (got["buffer_cand"] == 0xFF).all() and (got["full_count"] == 0).all()


@pytest.mark.skipif(not reference_available(), reason="the reference sources and oracle/_ref/obj_all are not here")
def test_restatement_matches_live_reference(tmp_path):
    import make_golden_md_fast as gen
    L = gen.build_driver(str(tmp_path))
    fx = mu.fixture()
    src = mu.source_planes()
    for z, (w, h) in enumerate(mu.SIZES):
        pool = mu.pool_planes(z, src)
        desc = mu.descriptors(z, N_DESC)
        for i, d in enumerate(desc):
            sads = gen.reference_sads(L, src, pool, d, w, h)     # asserts ASM_NON_AVX2 == ASM_AVX2
            assert sads == mu.candidate_sads(src, pool, d, w, h) == tuple(int(v) for v in fx[f"sads_z{z}"][i]), ((w, h), i)
            assert gen.reference_result(L, d, sads) == tuple(int(v) for v in np.ascontiguousarray(fx[f"result_z{z}"]).view(mu.RESULT_DTYPE)[i, 0]), ((w, h), i)
    result, desc, groups = mu.pick_inputs()
    picks = gen.reference_picks(L, result, desc, groups)         # asserts the restated PreModeDecision equal to the reference's
    assert np.array_equal(picks, mu.pick(result, desc, groups)[0])
    assert np.array_equal(picks.view(np.uint8).reshape(-1, 32), fx["pick"])
