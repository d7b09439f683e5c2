"""CPU: the restatement of the reference's CDEF (tests/cdef_util.py) against the fixture recorded from the reference itself
(tests/golden/cdef.npz, written by tests/golden/make_golden_cdef.py): the tables of the strength search, the counted flags, the directions
and variances of one fb, finish_cdef_search's result at three base_qindex values, av1_cdef_frame's output for the search's own result and
for two constructed ones, dist_8x8_16bit on the block pairs, and the constructed pick tables with their ties.  The coverage the fixture
claims is counted again while the restatement reproduces it.  Where the reference is present, one small case is checked against a fresh
run of the driver."""
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import cdef_util as cu  # noqa: E402

N_CASES = 6
_cache = {}


def fixture():
    if "z" not in _cache:
        _cache["z"] = dict(np.load(cu.fixture_path()))
    return _cache["z"]


def fixture_case(c):
    if c not in _cache:
        _cache[c] = cu.load_case(fixture(), c)
    return _cache[c]


def restated(c):
    """the restatement's search at every recorded qindex, with the coverage statistics: shared by the tests of this module"""
    key = ("restated", c)
    if key not in _cache:
        F = fixture_case(c)
        st = cu.new_stats()
        _cache[key] = ([cu.search(F["dbk"], F["src"], F["skip"], F["w"], F["h"], F["bd"], q, st) for q in F["qindex"]], st)
    return _cache[key]


@pytest.mark.parametrize("c", range(N_CASES))
def test_restatement_search_and_pick_equal_the_fixture(c):
    F = fixture_case(c)
    assert len(fixture()["case"]) == N_CASES
    for qi, q in enumerate(F["qindex"]):
        mse, counted, dirs, variances = restated(c)[0][qi]
        assert np.array_equal(mse, F["mse"][qi]), (c, q)
        assert np.array_equal(counted, F["counted"])
        res, fbs = cu.pick(F["mse"][qi], F["counted"], q, F["bd"])
        assert res == F["result"][qi] and np.array_equal(fbs, F["fb_strength"][qi]), (c, q)
        assert int(res["pri_damping"]) == 3 + (q >> 6)
    r0, c0 = F["dir_fb"] // F["nhfb"] * 8, F["dir_fb"] % F["nhfb"] * 8
    sub_d, sub_v = dirs[r0:r0 + 8, c0:c0 + 8], variances[r0:r0 + 8, c0:c0 + 8]
    got_d, got_v = F["dirs"].reshape(8, 8), F["vars"].reshape(8, 8)
    assert np.array_equal(got_d[:sub_d.shape[0], :sub_d.shape[1]], sub_d) and np.array_equal(got_v[:sub_v.shape[0], :sub_v.shape[1]], sub_v)


@pytest.mark.parametrize("c", range(N_CASES))
def test_restatement_frame_filter_equals_the_fixture(c):
    F = fixture_case(c)
    assert F["run_result"][0] == F["result"][0] and np.array_equal(F["run_fb_strength"][0], F["fb_strength"][0])
    for r in range(len(F["run_result"])):
        out = cu.frame(F["dbk"], F["skip"], F["w"], F["h"], F["bd"], F["run_result"][r], F["run_fb_strength"][r])
        for p in range(3):
            assert np.array_equal(out[p], F["out"][r][p]), (c, r, p)


@pytest.mark.parametrize("bd", (8, 10))
def test_restatement_dist_equals_the_fixture(bd):
    z = fixture()
    assert len(z[f"dist{bd}_ref"]) > 1500
    assert np.array_equal(cu.dist_8x8(z[f"dist{bd}_dst"], z[f"dist{bd}_src"], bd - 8), z[f"dist{bd}_ref"])


def test_synthetic_pick_tables_and_their_ties():
    z = fixture()
    assert set(z["synthetic"]) == {"syn_mse", "syn_counted", "syn_qindex", "syn_result", "syn_fb_strength"}
    want = z["syn_result"].view(cu.RESULT_DTYPE).reshape(-1)
    for t in range(len(z["syn_qindex"])):
        res, fbs = cu.pick(z["syn_mse"][t], z["syn_counted"][t], int(z["syn_qindex"][t]), 8)
        assert res == want[t] and np.array_equal(fbs, z["syn_fb_strength"][t]), t
    # every pair and every number of bits ties: the first pair in row-major order, the smallest i
    assert int(want[0]["cdef_bits"]) == 0 and int(want[0]["cdef_strengths"][0]) == 0 and int(want[0]["cdef_uv_strengths"][0]) == 0
    # four tied pairs (5 | 9) x (3 | 7): (5, 3)
    assert (int(want[1]["cdef_strengths"][0]), int(want[1]["cdef_uv_strengths"][0])) == (5, 3) and int(want[1]["cdef_bits"]) == 0


def test_fixture_covers_the_ground():
    """the arms of the issue's list, counted by the restatement while it reproduces the reference's recorded runs"""
    import make_golden_cdef as mg
    st = cu.new_stats()
    flags = {"partly_skipped_block_listed": False, "fb_all_skipped": False, "fb_single_block": False, "nothing_skipped": False, "var_zero": False,
             "sample_zero": False, "sample_max": False, "lambda_changes_bits": False, "narrow_fb": False, "low_fb": False}
    for c in range(N_CASES):
        F = fixture_case(c)
        runs, s = restated(c)
        for k in st:
            st[k] += s[k]
        for r in range(len(F["run_result"])):
            cu.frame(F["dbk"], F["skip"], F["w"], F["h"], F["bd"], F["run_result"][r], F["run_fb_strength"][r], st)
        listed, counted = cu.block_lists(F["skip"], F["w"], F["h"])
        s4 = F["skip"].reshape(listed.shape[0], 2, listed.shape[1], 2).sum((1, 3))
        flags["partly_skipped_block_listed"] |= bool(((s4 > 0) & (s4 < 4)).any())
        flags["fb_all_skipped"] |= bool((~counted).any())
        flags["fb_single_block"] |= any(listed[r * 8:(r + 1) * 8, k * 8:(k + 1) * 8].sum() == 1 for r in range(F["nvfb"]) for k in range(F["nhfb"]))
        flags["nothing_skipped"] |= not F["skip"].any()
        flags["var_zero"] |= bool(((runs[0][3] == 0) & listed).any())
        flags["sample_zero"] |= bool((F["dbk"][0] == 0).any())
        flags["sample_max"] |= bool((F["dbk"][0] == (1 << F["bd"]) - 1).any())
        flags["narrow_fb"] |= F["w"] % 64 == 8
        flags["low_fb"] |= F["h"] % 64 == 8
        for qi, q in enumerate(F["qindex"]):
            flags["lambda_changes_bits"] |= int(cu.pick(F["mse"][qi], F["counted"], q, F["bd"], lam=0.0)[0]["cdef_bits"]) != int(F["result"][qi]["cdef_bits"])
        assert len({3 + (q >> 6) for q in F["qindex"]}) >= 3
    assert mg.coverage(st, flags) == [], (st, flags)
    assert list(fixture()["coverage_keys"]) == list(cu.STAT_KEYS) + list(flags)


def test_restatement_against_a_fresh_run_of_the_driver():
    import make_golden_cdef as mg
    if not mg.reference_available():
        pytest.skip("the reference and its objects exist in the build container only")
    F = fixture_case(0)
    rng = np.random.default_rng(5)
    skip = (rng.random(F["skip"].shape) < 0.4).astype(np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        R = mg.Reference(mg.build_driver(tmp), F["w"], F["h"], F["bd"], F["dbk"], F["src"], skip)
        q = 140
        ref_mse = R.search(q)
        ref_res, ref_fbs = R.finish(q)
        ref_out = R.frame(ref_res, ref_fbs)
        R.close()
    mse, counted, _, _ = cu.search(F["dbk"], F["src"], skip, F["w"], F["h"], F["bd"], q)
    res, fbs = cu.pick(mse, counted, q, F["bd"])
    out = cu.frame(F["dbk"], skip, F["w"], F["h"], F["bd"], res, fbs)
    assert np.array_equal(mse, ref_mse) and res == ref_res and np.array_equal(fbs, ref_fbs)
    assert all(np.array_equal(a, b) for a, b in zip(out, ref_out))
