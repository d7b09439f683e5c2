"""CPU, with the reference present (skips without it): the numpy restatement of the film-grain Wiener denoising (tests/fg_denoise_util.py)
against the live driver (tests/golden/ref_fg_denoise_driver.c): block extraction at block size 16 and 32 at negative and past-the-edge
offsets, the forward transform's spectrum, the inverse transform of a spectrum, forward + filter + inverse of a block -- each compared as
raw bits -- then aom_wiener_denoise_2d on every case, the default psd, and the fixture regenerated equal to the committed one."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), ROOT]

import fg_denoise_util as du  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

pytestmark = pytest.mark.skipif(not reference_available(), reason="needs the reference sources and oracle/_ref/obj_all")


@pytest.fixture(scope="module")
def gen():
    import make_golden_fg_denoise
    return make_golden_fg_denoise


@pytest.fixture(scope="module")
def driver(gen, tmp_path_factory):
    return gen.build_driver(str(tmp_path_factory.mktemp("fg_denoise_ref")))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("n", (16, 32))
def test_transforms_and_filter_as_bits(gen, driver, n):
    rng = np.random.default_rng(n)
    H = n // 2
    for t in range(24):
        b = (rng.standard_normal((n, n)) * (10.0 ** rng.integers(-4, 2))).astype(np.float32)
        if t == 0:
            b[:] = 0
            b[3, 4] = -0.0
        if t == 1:
            b[:] = np.float32(1e-30)   # products underflow to denormals
        rr, ri = gen.reference_fft(driver, b)
        re, im = du.fft2d(b)
        assert np.array_equal(_bits(re), _bits(rr[:, :H + 1])) and np.array_equal(_bits(im), _bits(ri[:, :H + 1])), ("forward", t)
        assert np.array_equal(_bits(du.ifft2d(re, im)), _bits(gen.reference_ifft(driver, re, im))), ("inverse", t)
        for kind in ("nonflat", "default", "zero"):
            psd = du.psd_of(kind, t)[0 if n == 32 else 1]
            assert np.array_equal(_bits(du.tx_block(b, psd)), _bits(gen.reference_tx(driver, b, psd))), ("forward, filter, inverse", t, kind)


@pytest.mark.parametrize("p", range(len(du.PICTURES)))
def test_extraction_at_any_offset_as_bits(gen, driver, p):
    w, h, bd = du.PICTURES[p]
    data = du.planes_of(p)
    for c in (0, 1):
        n, pw, ph = 32 >> c, w >> c, h >> c
        for ox, oy in ((-n, -n), (-n // 2, 0), (0, -n // 2), (pw - 3, ph - n // 2), (pw, ph - 1), (5, ph + n), (n // 2, n // 2)):
            fit, block = gen.reference_block(driver, bd, n, data[c], ox, oy)
            mine_fit, mine_block = du.extract_blocks(data[c], bd, n, [(ox, oy)])
            assert np.array_equal(_bits(fit), _bits(mine_fit[:, 0])) and np.array_equal(_bits(block), _bits(mine_block[:, 0])), (p, c, ox, oy)


def test_default_psd(driver):
    for n in (16, 32):
        for f in (5.0, 0.5, 1.3, 7.25, 50.0):
            assert np.float32(driver.drv_fgd_psd(n, f)).view(np.uint32) == du.psd_default(n, f).view(np.uint32)


@pytest.mark.parametrize("k", range(len(du.CASES)))
def test_denoise_matches_the_live_reference_and_the_fixture(gen, driver, k):
    fx = du.fixture()
    p, content, kind = du.CASES[k]
    w, h, bd = du.PICTURES[p]
    data, psd = du.planes_of(p, content), du.psd_of(kind, k)
    ref = gen.reference_denoise(driver, bd, data, psd)
    planes, mine = du.denoise(data, bd, psd)
    for c in range(3):
        assert np.array_equal(ref[c], mine[c]) and np.array_equal(ref[c], fx[f"den_{k}_{c}"]), (k, c)
        assert np.array_equal(du.digest(du.picture_area(planes, w, h)[c]), fx[f"result_sha_{k}_{c}"]), (k, c)


def test_the_fixture_regenerated_equals_the_committed_one(gen, tmp_path, monkeypatch):
    committed = du.fixture()
    monkeypatch.setattr(du, "FIXTURE", str(tmp_path / "fg_denoise.npz"))
    gen.main()
    fresh = np.load(str(tmp_path / "fg_denoise.npz"))
    assert sorted(fresh.files) == sorted(committed.files)
    for name in committed.files:
        assert fresh[name].dtype == committed[name].dtype and np.array_equal(fresh[name], committed[name]), name
