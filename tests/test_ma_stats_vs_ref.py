"""CPU: the restatement of the motion-analysis statistics (tests/ma_stats_util.py) against the reference's own functions -- against the
recorded fixture (tests/golden/ma_stats.npz) everywhere, and against the live driver (tests/golden/ref_ma_stats_driver.c) where the
reference is available.  The fixture's coverage list is the generator's; a few of its conditions are read again from the recorded data."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import ma_stats_util as mu  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


def test_fixture_has_the_cases():
    z = mu.fixture()
    assert [tuple(int(v) for v in c) for c in z["case"]] == list(mu.CASES)
    assert len(z["coverage_keys"]) > 50
    assert os.path.getsize(mu.FIXTURE) < 1 << 20
    for w, h, groups in mu.fixture_cases():
        n = mu.n_sbs(w, h)
        assert len(groups["zz"]) >= 2 and len(groups["energy"]) == 7 and len(groups["tables"]) >= 8
        for item in groups["zz"]:
            assert item["cur"].shape == item["prev"].shape == (h, w) and item["sad"].shape == (n,)
        for item in groups["tables"]:
            assert item["me"].shape == (n, 85) and item["cand"].shape == (n, 85, 18) and item["flags"].shape == (n, 4)


@pytest.mark.parametrize("c", range(len(mu.CASES)))
def test_restatement_matches_fixture(c):
    w, h, groups = mu.fixture_cases()[c]
    for i, item in enumerate(groups["zz"]):
        for k, got in zip(mu.ZZ_KEYS[2:], mu.zz_sad(item["cur"], item["prev"])):
            assert got.dtype == item[k].dtype and np.array_equal(got, item[k]), ((w, h), "zz", i, k)
    for i, item in enumerate(groups["energy"]):
        for k, got in zip(mu.ENERGY_KEYS[3:], mu.ac_energy(item["luma"], int(item["intra"]), item["y_mean"])):
            assert got.dtype == item[k].dtype and np.array_equal(got, item[k]), ((w, h), "energy", i, k)
    for i, item in enumerate(groups["tables"]):
        mine = mu.all_tables(item, w, h)
        assert np.array_equal(mine["flags"], item["flags"]), ((w, h), "tables", i)
        if item["compare_global_motion"]:
            assert np.array_equal(mine["global_motion"][:6], item["global_motion"]) and mine["global_motion"][11] == 0, ((w, h), "tables", i)
        else:
            assert mine["global_motion"][11] > 0


def test_fixture_covers_the_ladders_and_both_arms():
    sads, zz, nm, gm, flags, intervals, intra_arm = set(), set(), set(), set(), set(), set(), False
    for w, h, groups in mu.fixture_cases():
        complete = mu.complete_sbs(w, h)
        for item in groups["zz"]:
            sads |= set(int(v) for v in item["sad"])
            zz |= set(int(v) for v in item["zz_cost"])
            nm |= set(int(v) for v in item["non_moving_index"])
        for item in groups["tables"]:
            s = mu.signals_dict(item["signals"])
            intra_arm |= bool(s["slice_is_intra"])
            if item["compare_global_motion"] and not s["slice_is_intra"]:
                gm.add((int(item["global_motion"][0]), int(item["global_motion"][1])))
            flags |= set((f, int(v)) for f in range(4) for v in item["flags"][complete, f])
            mine = mu.all_tables(item, w, h)
            intervals |= set(int(v) for v in mine["inter_index"][complete]) | set(int(v) for v in mine["intra_index"][complete])
    assert {255, 256, 511, 512, 1023, 1024, 2047, 2048, 0, 0xffffffff} <= sads
    assert zz == {0, 3, 10, 20, 30, 255} and nm == {0, 10, 20, 30}
    assert {(1, 0), (0, 1), (0, 0)} <= gm and intra_arm
    assert flags == {(f, v) for f in range(4) for v in (0, 1)}
    assert 127 in intervals and any(0 < v <= 63 for v in intervals) and any(63 < v < 127 for v in intervals)


def test_the_64x64_energy_is_not_the_sum_of_the_four():
    """the DC sum is shifted once per block group: four groups lose up to 3/4 each, the whole SB once"""
    w, h, groups = mu.fixture_cases()[0]
    e = groups["energy"][2]["energy"][0]
    assert int(e[0]) != int(e[1:].sum()) and abs(int(e[0]) - int(e[1:].sum())) <= 3


def test_division_truncates_towards_zero():
    assert mu._cdiv(-87, 2) == -43 and mu._cdiv(87, 2) == 43 and mu._cdiv(-40000 * 3, 3) == -40000 + 65536


@pytest.mark.skipif(not reference_available(), reason="the reference sources and oracle/_ref/obj_all are not here")
def test_restatement_matches_live_reference(tmp_path):
    import make_golden_ma_stats as gen
    L = gen.build_driver(str(tmp_path))
    for w, h, groups in mu.fixture_cases():
        for i, item in enumerate(groups["zz"]):
            ref = gen.reference_zz(L, w, h, item["cur"], item["prev"])
            for k, r, m in zip(mu.ZZ_KEYS[2:], ref, mu.zz_sad(item["cur"], item["prev"])):
                assert np.array_equal(r, m) and np.array_equal(r, item[k]), ((w, h), "zz", i, k)
        for i, item in enumerate(groups["energy"]):
            ref = gen.reference_energy(L, w, h, item["luma"], int(item["intra"]), item["y_mean"])
            for k, r, m in zip(mu.ENERGY_KEYS[3:], ref, mu.ac_energy(item["luma"], int(item["intra"]), item["y_mean"])):
                assert np.array_equal(r, m) and np.array_equal(r, item[k]), ((w, h), "energy", i, k)
        for i, item in enumerate(groups["tables"]):
            gm, flags = gen.reference_tables(L, w, h, item)
            mine = mu.all_tables(item, w, h)
            assert np.array_equal(flags, mine["flags"]) and np.array_equal(flags, item["flags"]) and np.array_equal(gm, item["global_motion"]), ((w, h), i)
            if item["compare_global_motion"]:
                assert np.array_equal(gm, mine["global_motion"][:6]), ((w, h), "tables", i)
