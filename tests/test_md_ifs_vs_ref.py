"""CPU: the restatement of mode decision's interpolation-filter search (tests/md_ifs_util.py) against the reference -- against the recorded
fixture (tests/golden/md_ifs.npz) everywhere, and against the live driver (tests/golden/ref_interp_search_driver.c: the reference's
highbd_variance64 in C and AVX2, av1_model_rd_from_var_lapndz, model_rd_from_sse and interpolation_filter_search itself) where the reference
is available.  Also: the generated model tables are what tools/gen_model_rd_tables.py renders, and every knot of them is pinned by a row of
the fixture."""
import os
import sys
import tempfile
import zlib

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")]

import gen_model_rd_tables as tables  # noqa: E402
import md_ifs_util as mu  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

N_DESC, N_SEARCH = 13, 32


def _crcs(planes):
    return [zlib.crc32(np.ascontiguousarray(p).tobytes()) for p in planes]


def _rows(a, dtype):
    return np.ascontiguousarray(a).view(dtype).reshape(-1)


def test_fixture_has_the_cases():
    z = mu.fixture()
    assert [tuple(int(v) for v in s) for s in z["sizes"]] == list(mu.SIZES) and len(set(mu.SIZES)) == 17 and all(min(s) > 4 for s in mu.SIZES)
    assert [tuple(int(v) for v in s) for s in z["search_sizes"]] == list(mu.SEARCH_SIZES)
    assert list(z["quantizers"]) == list(mu.QUANTIZERS) and int(z["max_quantizer"]) == mu.QUANTIZERS[-1]
    assert os.path.getsize(mu.FIXTURE) <= 200_000
    assert list(z["crc_src"]) == _crcs(mu.mfu.source_planes())
    pics = mu.search_pictures()
    assert list(z["crc_search"]) == _crcs([pics[0].y, pics[0].cb, pics[0].cr, pics[1].y, pics[1].cb, pics[1].cr, *pics[2]])
    for zi, size in enumerate(mu.SEARCH_SIZES):
        pu, f = mu.search_cases(size, N_SEARCH)
        assert int(z["crc_cases"][zi]) == zlib.crc32(pu.tobytes() + f.tobytes())
        assert {int(d) for d in pu["pred_direction"]} == {0, 1, 2}
    # the conditions on the search cases, read off the reference's rows
    full = np.concatenate([_rows(z[f"search_{w}x{h}_full"], mu.IFS_RESULT_DTYPE)["best_trial"] for w, h in mu.SEARCH_SIZES])
    fast = np.concatenate([_rows(z[f"search_{w}x{h}_fast"], mu.IFS_RESULT_DTYPE)["best_trial"] for w, h in mu.SEARCH_SIZES])
    no_dual = np.concatenate([_rows(z[f"search_{w}x{h}_no_dual"], mu.IFS_RESULT_DTYPE)["best_trial"] for w, h in mu.SEARCH_SIZES])
    assert set(full.tolist()) == set(range(9)) and set(fast.tolist()) == {0, 3, 6} and set(no_dual.tolist()) == {0, 4, 8}
    skip = np.concatenate([_rows(z[f"search_{w}x{h}_{m}"], mu.IFS_RESULT_DTYPE)["skip_txfm_sb"] for w, h in mu.SEARCH_SIZES for m, _, _ in mu.MODES])
    assert skip.sum() == 2 * len(mu.SEARCH_SIZES) * len(mu.MODES)


def test_model_tables():
    """the .inc is what the tool renders; the knots follow their closed form; every one of the 104 entries of both tables is pinned by a row
    of the fixture that lands on it exactly (the last one as the upper end of the last interval)"""
    with open(os.path.join(ROOT, "svt-av1-1_amd", "csrc", "md_model_rd_tables.inc")) as f:
        assert f.read() == tables.render(), "run tools/gen_model_rd_tables.py"
    assert len(tables.XSQ) == len(tables.RATE) == len(tables.DIST) == 104
    assert tables.XSQ[:10] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40] and tables.XSQ[-1] == 245728 and tables.RATE[0] == 65536 and tables.DIST[0] == 0
    assert all(a > b for a, b in zip(tables.RATE[:98], tables.RATE[1:99])) and all(a <= b for a, b in zip(tables.DIST, tables.DIST[1:]))
    z = mu.fixture()
    knots = z["lapndz_knot"]
    assert sorted(int(k) for k in knots if k >= 0) == list(range(104))
    for (var, n_log2, qstep), (rate, dist), knot in zip(z["lapndz_in"], z["lapndz_out"], knots):
        assert mu.model_rd_from_var_lapndz(int(var), int(n_log2), int(qstep)) == (int(rate), int(dist)), (var, n_log2, qstep)
        if 0 < knot < 103:   # on a knot the interpolation weights are 1024 and 0: the row shows the table entries themselves
            xsq = min((((int(qstep) ** 2) << (int(n_log2) + 10)) + (int(var) >> 1)) // int(var), mu.MAX_XSQ_Q10)
            assert xsq == tables.XSQ[knot]
            assert (int(rate), int(dist)) == (((tables.RATE[knot] << int(n_log2)) + 1) >> 1, (int(var) * tables.DIST[knot] + 512) >> 10)
    assert (z["lapndz_in"][:, 0] == 0).sum() >= 2 and (z["lapndz_in"][:, 2] == 0).sum() >= 2 and (z["lapndz_in"][:, 2] == mu.QUANTIZERS[-1] >> 3).sum() >= 8


def test_model_rd_from_sse_matches_fixture():
    z = mu.fixture()
    log2_of = {b: mu.log2(w * h) for (w, h), b in mu.BSIZE.items()}
    log2_of.update({0: 4, 1: 5, 2: 5, 16: 6, 17: 6})
    assert len(z["from_sse_in"]) == 17 * N_DESC * 3 * len(mu.QUANTIZERS)
    for (bsize, quantizer, sse), (rate, dist) in zip(z["from_sse_in"], z["from_sse_out"]):
        assert mu.model_rd_from_sse(log2_of[int(bsize)], int(quantizer), int(sse)) == (int(rate), int(dist)), (bsize, quantizer, sse)


@pytest.mark.parametrize("z", range(len(mu.SIZES)))
def test_model_rd_matches_fixture(z):
    fx = mu.fixture()
    w, h = mu.SIZES[z]
    src, pool = mu.model_planes(z)
    assert list(fx["crc_pool"][z]) == _crcs(pool)
    desc = mu.model_descriptors(z, N_DESC)
    for i, d in enumerate(desc):
        assert mu.tile_sses(src, pool, d, w, h) == [int(v) for v in fx[f"sse_z{z}"][i]], ((w, h), i)
    for k, quantizer in enumerate(mu.QUANTIZERS):
        got, refused = mu.model_rd(src, pool, desc, w, h, quantizer)
        assert refused == 0 and np.array_equal(got, _rows(fx[f"model_z{z}_q{k}"], mu.MODEL_RESULT_DTYPE)), ((w, h), quantizer)
    assert (desc["rate"] < 0).any() and (desc["lambda_"] > 0x7FFFFFFF).any()


def test_model_rd_extreme_matches_fixture():
    fx = mu.fixture()
    s, p, d = mu.extreme_tile()
    assert mu.tile_sses(s, p, d[0], 128, 128) == [int(v) for v in fx["sse_extreme"]]
    assert np.array_equal(mu.model_rd(s, p, d, 128, 128, mu.QUANTIZERS[-1])[0], _rows(fx["model_extreme"], mu.MODEL_RESULT_DTYPE))


@pytest.mark.parametrize("size", mu.SEARCH_SIZES)
def test_search_matches_fixture(size):
    fx = mu.fixture()
    w, h = size
    _, _, trials = mu.search_trials(size, N_SEARCH, mu.search_quantizer(size))
    for name, search_mode, dual in mu.MODES:
        got, refused = mu.search(trials, search_mode, dual)
        want = _rows(fx[f"search_{w}x{h}_{name}"], mu.IFS_RESULT_DTYPE)
        bad = np.flatnonzero(got != want)
        assert refused == 0 and bad.size == 0, (size, name, bad[:4], got[bad[:2]], want[bad[:2]])
    # the walks measure what the reference measures: 3 + 2 calls in fast mode (the first two of them trial 0 again), 9 and 3 otherwise
    assert mu.search_one(trials[4], 1, 1)[1] == [0, 0, 0, 3, 6] and mu.search_one(trials[4], 2, 1)[1] == list(range(9))
    assert mu.search_one(trials[4], 2, 0)[1] == [0, 4, 8] and mu.search_one(trials[4], 1, 0)[1] == [0, 4, 8]


def test_walk_rules_by_hand():
    """strict <, the listed order, and the fast mode's first loop as a build with one-byte enums runs it"""
    def run(rds, mode, dual):
        return mu.walk(mode, dual, lambda t: (rds[t], 1, 0))[0]
    assert run([5] * 9, 2, 1) == 0 and run([5, 5, 5, 5, 4, 4, 4, 4, 4], 2, 1) == 4 and run([9, 8, 7, 6, 5, 4, 3, 2, 1], 2, 1) == 8
    assert run([9, 8, 7, 6, 5, 4, 3, 2, 1], 2, 0) == 8 and run([9, 1, 1, 1, 9, 1, 1, 1, 9], 2, 0) == 0 and run([9, 1, 1, 1, 8, 1, 1, 1, 8], 1, 0) == 4
    assert run([9, 1, 1, 8, 1, 1, 7, 1, 1], 1, 1) == 6 and run([9, 1, 1, 9, 1, 1, 9, 1, 1], 1, 1) == 0 and run([9, 1, 1, 8, 0, 0, 8, 0, 0], 1, 1) == 3
    assert run([-5, 0, 0, -6, 0, 0, -(1 << 62), 0, 0], 1, 1) == 6


@pytest.mark.skipif(not reference_available(), reason="needs the reference sources and oracle/_ref/obj_all")
def test_live_reference_agrees():
    """a few rows of every kind recomputed by the reference now, on inputs the fixture does not hold (another variant of the cases)"""
    import make_golden_md_ifs as gen
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(tmp)
        for v, n, q in ((777, 6, 33), (123456789, 12, 150), (5, 4, 228), (0, 8, 9)):
            assert gen.reference_lapndz(L, v, n, q) == mu.model_rd_from_var_lapndz(v, n, q)
        z = mu.SIZES.index((32, 16))
        src, pool = mu.model_planes(z)
        for d in mu.model_descriptors(z, 7, variant=3):
            assert gen.reference_sses(L, src, pool, d, 32, 16) == mu.tile_sses(src, pool, d, 32, 16)
        pics = mu.search_pictures()
        for size in ((16, 8), (32, 32)):
            quantizer = 333
            pu, f, trials = mu.search_trials(size, 20, quantizer, variant=5)
            for name, search_mode, dual in mu.MODES:
                mine, _ = mu.search(trials, search_mode, dual)
                for k in range(len(pu)):
                    assert gen.reference_search(L, pics, pu[k], f[k], size[0], size[1], quantizer, search_mode, dual) == mine[k], (size, name, k)
