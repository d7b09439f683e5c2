"""CPU: the restatement of the picture-analysis statistics (tests/pa_stats_util.py) against the reference's GatheringPictureStatistics --
against the recorded fixture (tests/golden/pa_stats.npz) everywhere, and against the live driver (tests/golden/ref_pa_stats_driver.c) where
the reference is available.  The fixture's coverage list is checked again here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import pa_stats_util as pu  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


def test_fixture_has_the_cases():
    z = pu.fixture()
    assert [tuple(int(v) for v in c) for c in z["case"]] == list(pu.CASES)
    for c, (w, h, pics) in enumerate(pu.fixture_cases()):
        assert len(pics) >= 8
        for luma, cb, cr, outs in pics:
            assert luma.shape == (h, w) and cb.shape == cr.shape == (h // 2, w // 2)
            assert all(set(outs[sub]) == set(pu.OUTPUTS) for sub in (0, 1))


@pytest.mark.parametrize("c", range(len(pu.CASES)))
def test_restatement_matches_fixture(c):
    w, h, pics = pu.fixture_cases()[c]
    for i, (luma, cb, cr, outs) in enumerate(pics):
        for sub in (0, 1):
            mine = pu.all_stats(luma, cb, cr, sub)
            for k in pu.OUTPUTS:
                assert mine[k].dtype == outs[sub][k].dtype and np.array_equal(mine[k], outs[sub][k]), ((w, h), i, sub, k)


def test_fixture_covers_the_ground():
    z = pu.fixture()
    assert tuple(z["coverage_keys"]) == pu.COVERAGE_KEYS
    cov = pu.coverage([(w, h, *pic) for (w, h, pics) in pu.fixture_cases() for pic in pics])
    assert all(cov.values()), [k for k, v in cov.items() if not v]


def test_flat_255_needs_more_than_31_bits():
    """the 8.8 mean of a flat block of 255 is 65280: its square passes 2^31, and the variance is still 0"""
    y, v, _, _ = pu.block_stats(np.full((64, 64), 255, np.uint8), np.zeros((32, 32), np.uint8), np.zeros((32, 32), np.uint8), 0)
    assert (y == 255).all() and (v == 0).all() and 65280 * 65280 > 2 ** 31


@pytest.mark.skipif(not reference_available(), reason="the reference sources and oracle/_ref/obj_all are not here")
def test_restatement_matches_live_reference(tmp_path):
    import make_golden_pa_stats as gen
    L = gen.build_driver(str(tmp_path))
    for (w, h, pics) in pu.fixture_cases():
        for i, (luma, cb, cr, outs) in enumerate(pics):
            ref = gen.reference_stats(L, luma, cb, cr)
            for sub in (0, 1):
                mine = pu.all_stats(luma, cb, cr, sub)
                for k in pu.OUTPUTS:
                    assert np.array_equal(mine[k], ref[sub][k]) and np.array_equal(outs[sub][k], ref[sub][k]), ((w, h), i, sub, k)
