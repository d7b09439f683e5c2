"""CPU: the restatement of the reference's CDEF on grids with 128-wide blocks (tests/cdef128_util.py) against the fixture recorded from the
reference itself (tests/golden/cdef128.npz, written by tests/golden/make_golden_cdef128.py): the tables and counted flags at three
base_qindex values, finish_cdef_search's result with the copies it makes, av1_cdef_frame's output for the search's own result and for a
constructed one; the coverage the fixture claims; case D against the 64x64 restatement.  Where the reference is present, the contradictory
case with another skip map is checked against a fresh run of the driver."""
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import cdef128_util as c128  # noqa: E402
import cdef_util as cu  # noqa: E402

N_CASES = len(c128.CASES)
_cache = {}


def fixture():
    if "z" not in _cache:
        _cache["z"] = dict(np.load(c128.fixture_path()))
    return _cache["z"]


def fixture_case(c):
    if c not in _cache:
        _cache[c] = c128.load_case(fixture(), c)
    return _cache[c]


def case_index(name, bd):
    return c128.CASES.index(next(k for k in c128.CASES if k[0] == name and k[3] == bd))


def quadrants(c, qi):
    """the restatement's sums per quadrant: B and D share a picture, so they share these"""
    F = fixture_case(c)
    key = ("quads", int(fixture()["case_picture"][c]), qi)
    if key not in _cache:
        _cache[key] = c128.quadrant_sums(F["dbk"], F["src"], F["skip"], F["w"], F["h"], F["bd"], F["qindex"][qi])
    return _cache[key]


@pytest.mark.parametrize("c", range(N_CASES))
def test_restatement_search_and_pick_equal_the_fixture(c):
    F = fixture_case(c)
    assert (F["name"], F["w"], F["h"], F["bd"]) == c128.CASES[c] and len(fixture()["case"]) == N_CASES
    assert np.array_equal(F["sb_type"], c128.make_grid(F["name"], F["w"], F["h"]))
    assert len({3 + (q >> 6) for q in F["qindex"]}) == 3
    for qi, q in enumerate(F["qindex"]):
        mse, counted = c128.merge(quadrants(c, qi), F["sb_type"], F["skip"], F["w"], F["h"], F["bd"])
        assert np.array_equal(mse, F["mse"][qi]) and np.array_equal(counted, F["counted"]), (c, q)
        res, fbs = c128.pick(F["mse"][qi], F["counted"], F["sb_type"], F["w"], F["h"], q, F["bd"])
        assert res == F["result"][qi] and np.array_equal(fbs, F["fb_strength"][qi]), (c, q)
        assert int(res["sb_count"]) == int(F["counted"].sum())


@pytest.mark.parametrize("c", range(N_CASES))
def test_restatement_frame_filter_equals_the_fixture(c):
    F = fixture_case(c)
    assert F["run_result"][0] == F["result"][0] and np.array_equal(F["run_fb_strength"][0], F["fb_strength"][0])
    assert int(F["run_result"][1]["pri_damping"]) != int(F["run_result"][1]["sec_damping"]) and int(F["run_result"][1]["nb_cdef_strengths"]) == 8
    for r in range(len(F["run_result"])):
        out = c128.frame(F["dbk"], F["skip"], F["w"], F["h"], F["bd"], F["run_result"][r], F["run_fb_strength"][r])
        for p in range(3):
            assert np.array_equal(out[p], F["out"][r][p]), (c, r, p)


def test_named_cases_are_what_the_fixture_says():
    A, B, C = (fixture_case(case_index(n, 8)) for n in "ABC")
    assert A["counted"].tolist() == [1, 0, 0, 0] and (A["fb_strength"] == A["fb_strength"][:, :1]).all() and (A["fb_strength"] >= 0).all()
    assert (B["nhfb"], B["nvfb"]) == (6, 4)
    assert C["counted"].tolist() == [1, 1, 1, 1]        # fbs 1, 2 and 3 are searched on their own
    for bd in (8, 10):                                    # the wide fb left out for its first 64x64: its twin stays -1
        B = fixture_case(case_index("B", bd))
        assert B["counted"][14] == 0 and (B["fb_strength"][:, 14:16] == -1).all()
        listed, _ = cu.block_lists(B["skip"], B["w"], B["h"])
        assert listed[16:24, 24:32].any()


@pytest.mark.parametrize("bd", (8, 10))
def test_case_d_equals_the_64x64_treatment(bd):
    F = fixture_case(case_index("D", bd))
    assert int(np.minimum(F["sb_type"], 21).max()) < c128.BLOCK_64X128
    B = fixture_case(case_index("B", bd))
    assert all(np.array_equal(a, b) for a, b in zip(F["dbk"], B["dbk"])) and np.array_equal(F["skip"], B["skip"])
    _, counted = cu.block_lists(F["skip"], F["w"], F["h"])
    assert np.array_equal(F["counted"], counted.reshape(-1))
    q = quadrants(case_index("D", bd), 0)
    s = np.uint64(2 * (bd - 8))
    assert np.array_equal(F["mse"][0][0], q[0] >> s) and np.array_equal(F["mse"][0][1], (q[1] >> s) + (q[2] >> s))
    for qi, qx in enumerate(F["qindex"]):
        res, fbs = cu.pick(F["mse"][qi], F["counted"], qx, bd)
        assert res == F["result"][qi] and np.array_equal(fbs, F["fb_strength"][qi])


def test_fixture_covers_the_ground():
    cases = [fixture_case(c) for c in range(N_CASES)]
    cov = c128.coverage(cases, lambda F: quadrants(next(c for c in range(N_CASES) if cases[c] is F), 0))
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    assert list(fixture()["coverage_keys"]) == list(c128.COVERAGE_KEYS)
    assert os.path.getsize(c128.fixture_path()) < 1 << 20


def test_restatement_against_a_fresh_run_of_the_driver():
    import make_golden_cdef128 as mg
    if not mg.reference_available():
        pytest.skip("the reference and its objects exist in the build container only")
    F = dict(fixture_case(case_index("C", 10)))
    rng = np.random.default_rng(5)
    F["skip"] = (rng.random(F["skip"].shape) < 0.4).astype(np.uint8)
    F["skip"][16:32, 0:16] = 1       # fb 2, which says 128X64: left out with its copy, fb 3 on its own
    F["qindex"] = [140]
    with tempfile.TemporaryDirectory() as tmp:
        R = mg.Reference(mg.build_driver(tmp), F["w"], F["h"], F["bd"], F["dbk"], F["src"], F["skip"], F["sb_type"])
        _, counted, res, fbs = mg.check_case(R, F, 0)
        mg.check_frame(R, F, res, fbs)
        R.close()
    assert counted.tolist() == [1, 1, 0, 1]
