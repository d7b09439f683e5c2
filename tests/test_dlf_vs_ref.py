"""The numpy restatement of the deblocking filter and its level search (tests/dlf_util.py) against the reference's own
av1_loop_filter_frame, PictureSseCalculations and av1_pick_filter_level, as recorded in tests/golden/dlf.npz and, where the reference
exists, live.  Also the proof the device kernels rest on: two whole-plane passes leave what the reference's superblock order leaves."""
import functools
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import dlf_util as du  # noqa: E402
import make_golden_dlf as gen  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "dlf.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


@functools.lru_cache(maxsize=None)
def fixture_cases():
    """[(c, w, h, bd, mi, recon[3], source[3], runs, outs[run][3])]"""
    z = fixture()
    cases = []
    for c, (w, h, bd) in enumerate(z["case"]):
        runs = [tuple(int(v) for v in r) for r in z[f"c{c}_run"]]
        cases.append((c, int(w), int(h), int(bd), z[f"c{c}_mi"].view(du.LF_MI_DTYPE).reshape(z[f"c{c}_mi"].shape[:2]),
                      [z[f"c{c}_recon_{p}"] for p in range(3)], [z[f"c{c}_source_{p}"] for p in range(3)], runs,
                      [[z[f"c{c}_out{r}_{p}"] for p in range(3)] for r in range(len(runs))]))
    return cases


def fixture_picks(c):
    """[(last levels, only 4x4, levels, trace, masks[5])] of case c"""
    z = fixture()
    return [(tuple(int(v) for v in row[:4]), int(row[4]), [int(v) for v in row[5:]], z[f"c{c}_pick{k}_trace"], z[f"c{c}_pick{k}_mask"])
            for k, row in enumerate(z[f"c{c}_pick"])]


def _filtered(case, run, literal):
    (_, w, h, bd, mi, recon, _, runs, _) = case
    l0, l1, lu, lv, sharpness, ps, pe = runs[run]
    planes = [p.copy() for p in recon]
    du.loop_filter_frame(planes, mi, (l0, l1, lu, lv), sharpness, ps, pe, bd, literal=literal)
    return planes


@pytest.mark.parametrize("c", range(6))
def test_reference_order_matches_fixture(c):
    """form (a), the reference's superblock order with its advancing walk, leaves what the reference left"""
    case = fixture_cases()[c]
    for r in range(len(case[7])):
        got = _filtered(case, r, True)
        for p in range(3):
            assert np.array_equal(got[p], case[8][r][p]), (c, r, p)


@pytest.mark.parametrize("c", range(6))
def test_two_passes_match_reference_order(c):
    """form (b) == form (a) == the reference: all vertical edges, then all horizontal edges, every edge of a pass independent"""
    case = fixture_cases()[c]
    for r in range(len(case[7])):
        a, b = _filtered(case, r, True), _filtered(case, r, False)
        for p in range(3):
            assert np.array_equal(a[p], b[p]), (c, r, p)
            assert np.array_equal(b[p], case[8][r][p]), (c, r, p)


def test_edges_of_a_pass_are_independent():
    """within one pass the order of the edges does not matter: lengths filtered 14 first or 4 first leave the same plane"""
    (_, w, h, bd, mi, recon, _, _, _) = fixture_cases()[1]
    for direction in (0, 1):
        a, b = recon[0].copy(), recon[0].copy()
        L = du.edge_lengths(mi, 0, direction, w, h, 30)
        for img, order in ((a, (4, 8, 14)), (b, (14, 8, 4))):
            for n in order:
                uy, ux = np.nonzero(L == n)
                du.apply_edges(img, uy, ux, n, direction, 30, 0, bd)
        assert np.array_equal(a, b)


@pytest.mark.parametrize("c", range(6))
def test_sse_tables_match_fixture(c):
    (_, w, h, bd, mi, recon, source, _, _) = fixture_cases()[c]
    z = fixture()
    for i, (plane, direction, _, _) in enumerate(du.PICK_RUNS):
        levels = [int(v) for v in z[f"c{c}_table_levels"][i]]
        got = du.sse_table(recon, source, mi, plane, direction, levels, 0, bd)
        assert [got[k] for k in range(64)] == [int(v) for v in z[f"c{c}_table"][i]], (c, plane, direction)


@pytest.mark.parametrize("c", range(6))
def test_pick_matches_fixture(c):
    """levels, every filtering the reference ran (in its order) and the walks' masks"""
    (_, w, h, bd, mi, recon, source, _, _) = fixture_cases()[c]
    for (last, only, want, trace, masks) in fixture_picks(c):
        levels, got_masks, got_trace = du.pick_filter_level(recon, source, mi, last, 0, only, bd)
        assert levels == want, (c, last, only)
        assert np.array_equal(np.array(got_trace), trace), (c, last, only)
        assert [int(m) for m in masks] == got_masks


def test_walks_match_fixture():
    z = fixture()
    n_ref = 0
    for t, (start, only), (want, mask), syn in zip(z["walk_table"], z["walk_arg"], z["walk_out"], z["walk_synthetic"]):
        best, got_mask, _ = du.level_walk(t, int(start), int(only))
        assert (best, got_mask) == (int(want), int(mask))
        n_ref += not syn
    assert n_ref >= 50


def test_fixture_covers_the_ground():
    z = fixture()
    cases = [(w, h, bd, mi, recon, source) for (_, w, h, bd, mi, recon, source, _, _) in fixture_cases()]
    assert [(w, h, bd) for (w, h, bd, *_) in cases] == [(w, h, bd) for bd in (8, 10) for (w, h) in gen.SIZES]
    assert all(tuple(r) == g for (_, _, _, _, _, _, _, runs, _) in fixture_cases() for r, g in zip(runs, gen.RUNS))
    ws = {0: du.new_walk_stats(), 1: du.new_walk_stats()}
    for t, (start, only), syn in zip(z["walk_table"], z["walk_arg"], z["walk_synthetic"]):
        du.level_walk(t, int(start), int(only), ws[int(only)])
    for c in range(6):
        (_, w, h, bd, mi, recon, source, _, _) = fixture_cases()[c]
        for (last, only, _, _, _) in fixture_picks(c):
            du.pick_filter_level(recon, source, mi, last, 0, only, bd, st=ws[only])
    assert gen.coverage(cases, ws) is None


@pytest.mark.skipif(not gen.reference_available(), reason="needs the reference sources and oracle/_ref/obj_all")
def test_live_against_reference():
    """a fresh picture: frame filter (both forms), one table and the pick against the reference itself"""
    rng = np.random.default_rng(77)
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(tmp)
        for bd in (8, 10):
            mi, recon, source = gen.make_case(rng, 136, 72, bd)
            for levels, sharpness in (((17, 44, 9, 31), 0), ((5, 0, 63, 2), 6)):
                want = gen.reference_filter(L, bd, mi, recon, levels, sharpness, 0, 3)
                for literal in (True, False):
                    got = [p.copy() for p in recon]
                    du.loop_filter_frame(got, mi, levels, sharpness, 0, 3, bd, literal=literal)
                    assert all(np.array_equal(g, w) for g, w in zip(got, want)), (bd, levels, literal)
            want = gen.reference_table(L, bd, mi, recon, source, 0, 1, (21, 0, 0, 0))
            got = du.sse_table(recon, source, mi, 0, 1, (21, 0, 0, 0), 0, bd)
            assert [got[k] for k in range(64)] == [int(v) for v in want]
            lv, trace = gen.reference_pick(L, bd, mi, recon, source, (9, 30, 18, 40), 0)
            o_lv, _, o_trace = du.pick_filter_level(recon, source, mi, (9, 30, 18, 40), 0, 0, bd)
            assert o_lv == lv and np.array_equal(np.array(o_trace), trace)
