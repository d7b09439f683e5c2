"""CPU: the restatement of noise detection and denoising (tests/pa_noise_util.py) against the reference's FullSampleDenoise -- against the
recorded fixture (tests/golden/pa_noise.npz) everywhere, and against the live driver (tests/golden/ref_pa_noise_driver.c, ASM_AVX2 and the C
function pointers, denoiseFlag 0 and 1) where the reference is available.  The fixture's coverage list is checked again here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import pa_noise_util as nu  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


def test_fixture_has_the_cases():
    z = nu.fixture()
    assert [tuple(int(v) for v in c) for c in z["case"]] == list(nu.CASES)
    assert os.path.getsize(nu.FIXTURE) <= 450_000
    for c, (w, h, pics) in enumerate(nu.fixture_cases()):
        assert len(pics) >= 6
        for luma, cb, cr, outs in pics:
            assert luma.shape == (h, w) and cb.shape == cr.shape == (h // 2, w // 2)
            assert all(set(outs[sub]) == set(nu.FIXTURE_OUTPUTS) for sub in (0, 1))


@pytest.mark.parametrize("c", range(len(nu.CASES)))
def test_restatement_matches_fixture(c):
    w, h, pics = nu.fixture_cases()[c]
    for i, (luma, cb, cr, outs) in enumerate(pics):
        for sub in (0, 1):
            mine = nu.detect(luma, sub)
            for k in nu.DETECT_OUTPUTS + ("denoised",):
                assert mine[k].dtype == outs[sub][k].dtype and np.array_equal(mine[k], outs[sub][k]), ((w, h), i, sub, k)
            for k, p in zip(("out_luma", "out_cb", "out_cr"), nu.denoise(luma, cb, cr, mine)):
                assert p.dtype == np.uint8 and np.array_equal(p, outs[sub][k]), ((w, h), i, sub, k)


def test_fixture_covers_the_ground():
    z = nu.fixture()
    assert tuple(z["coverage_keys"]) == nu.COVERAGE_KEYS
    cov = nu.coverage([(w, h, *pic) for (w, h, pics) in nu.fixture_cases() for pic in pics])
    assert all(cov.values()), [k for k, v in cov.items() if not v]


def test_class_ladder_and_clamp():
    """every rung under both thresholds; classes 4 and above come back as 3_1"""
    for height, th in ((720, 25), (728, 0)):
        rungs = [(0, 1), (4 + th, 1), (5 + th, 2), (9 + th, 2), (10 + th, 3), (16 + th, 3), (17 + th, 4), (19 + th, 4)]
        assert [nu.noise_class(a, height)[0] for a, _ in rungs] == [c for _, c in rungs]
        for a, raw in ((20 + th, 5), (30 + th, 6), (40 + th, 7), (50 + th, 8), (60 + th, 9), (70 + th, 10), (80 + th, 11), (4096, 11)):
            assert nu.noise_class(a, height) == (nu.CLASS_3_1, raw)


def test_outermost_samples_are_copied_and_noise_clips():
    rng = np.random.default_rng(3)
    luma = rng.integers(0, 256, (72, 136)).astype(np.uint8)
    den, noise = nu.weak_luma(luma)
    for edge in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        assert np.array_equal(den[edge], luma[edge]) and (noise[edge] == 0).all()
    inner = np.s_[1:-1, 1:-1]
    assert ((luma[inner] < den[inner]) == ((noise[inner] == 0) & (luma[inner] != den[inner]))).all() and (luma[inner] < den[inner]).any()


@pytest.mark.skipif(not reference_available(), reason="the reference sources and oracle/_ref/obj_all are not here")
def test_restatement_matches_live_reference(tmp_path):
    import make_golden_pa_noise as gen
    L = gen.build_driver(str(tmp_path))
    for (w, h, pics) in nu.fixture_cases():
        for i, (luma, cb, cr, outs) in enumerate(pics):
            ref = gen.reference_noise(L, luma, cb, cr)     # asserts ASM_AVX2 == C path and denoiseFlag 0 == 1 on what both leave
            for sub in (0, 1):
                mine = nu.detect(luma, sub)
                planes = dict(zip(("out_luma", "out_cb", "out_cr"), nu.denoise(luma, cb, cr, mine)))
                for k in nu.FIXTURE_OUTPUTS:
                    got = planes[k] if k in planes else mine[k]
                    assert np.array_equal(got, ref[sub][k]) and np.array_equal(outs[sub][k], ref[sub][k]), ((w, h), i, sub, k)
