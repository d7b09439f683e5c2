"""CPU: the numpy restatement of the self-guided restoration search and frame filter (tests/lr_sgr_util.py) equals the reference's own run
recorded in tests/golden/lr_sgr.npz (tests/golden/make_golden_lr_sgr.py): the box filter's output, the five sums, the solve, the walk trial
by trial, the result per unit, the SSE, the frame runs; the constructed cases give what the fixture says; the fixture covers the ground.
Where the reference and the oracle build exist, the maker's whole comparison against the driver runs as well (slow, so one case)."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import lr_sgr_util as su  # noqa: E402
import lr_util as lu  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "lr_sgr.npz")
N_CASES = 8


@functools.lru_cache(maxsize=None)
def fixture():
    assert os.path.exists(FIXTURE), "tests/golden/lr_sgr.npz is missing (python tests/golden/make_golden_lr_sgr.py in the build container)"
    return dict(np.load(FIXTURE))


@functools.lru_cache(maxsize=None)
def lr_fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "lr.npz")))


@functools.lru_cache(maxsize=None)
def fixture_case(c):
    return su.load_case(fixture(), lr_fixture(), c)


def walk_table(coef, quant):
    x0 = np.arange(su.PRJ_MIN[0], su.PRJ_MAX[0] + 1, dtype=np.int64)[:, None]
    x1 = np.arange(su.PRJ_MIN[1], su.PRJ_MAX[1] + 1, dtype=np.int64)[None, :]
    e = coef[0][0] * (x0 - coef[0][1]) ** 2 + coef[0][2] * np.abs(x0 - coef[0][1]) + coef[1][0] * (x1 - coef[1][1]) ** 2 + coef[1][2] * np.abs(x1 - coef[1][1])
    return np.ascontiguousarray(1000 + e // int(quant) * int(quant))


def test_fixture_has_the_cases():
    z = fixture()
    assert [int(v) for v in z["lr_case"]] == [0, 1, 2, 4, 5, 6, -1, -1]
    assert [(fixture_case(c)["w"], fixture_case(c)["h"], fixture_case(c)["bd"]) for c in range(N_CASES)] == \
        [(64, 64, 8), (200, 136, 8), (136, 200, 8), (64, 64, 10), (200, 136, 10), (136, 200, 10), (64, 64, 8), (64, 64, 10)]
    for c in (6, 7):
        F = fixture_case(c)
        assert len(np.unique(F["cdef"][1])) == 1 and np.array_equal(F["cdef"][2], F["src"][2])


@pytest.mark.parametrize("c", range(N_CASES))
def test_search_matches_reference(c):
    """per unit: the five sums, exq, start, every trial of every walk, the final xqd and error, the best set, the SSE of its filter"""
    F = fixture_case(c)
    cap = int(fixture()["trace_cap"])
    traces = su.case_traces(F, cap)
    for p in range(3):
        for i, lim in enumerate(F["limits"][p]):
            u = F["base"][p] + i
            det, mine, best = su.search_unit(F["cdef"][p], F["src"][p], lim, F["bd"], int(p > 0))
            for k in det.dtype.names:
                assert np.array_equal(det[k], F["detail"][u][k]), (c, u, k)
            for ep in range(16):
                got = [(su.decode_xq(q, ep), e) for (q, e) in mine[ep][:cap]]
                assert got == traces[(u, ep)], (c, u, ep)
            assert list(best) == [int(v) for v in F["sgrproj"][u][:3]] and F["sgrproj"][u][3] == 0
            assert su.trial_sse(F["cdef"][p], F["dbk"][p], F["src"][p], lim, best[0], best[1:], F["bd"], int(p > 0)) == int(F["sse"][u])
    assert int(F["detail"]["n_trials"].max()) <= su.max_walk_trials()


@pytest.mark.parametrize("c", range(N_CASES))
def test_box_filter_matches_reference(c):
    """sum flt and sum flt^2 per plane and set; the samples themselves for the 64x64 pictures at one set per arm"""
    F = fixture_case(c)
    dump_ep = [int(v) for v in fixture()["dump_ep"]]
    for p in range(3):
        at = sum(F["cdef"][q].size for q in range(p))
        for ep in range(16):
            flt = su.plane_flt(F["cdef"][p], F["limits"][p], F["bd"], ep, int(p > 0))
            mine = [v for k in range(2) for v in ((int(flt[k].sum()), int((flt[k] * flt[k]).sum())) if flt[k] is not None else (0, 0))]
            assert mine == [int(v) for v in F["fsums"][p][ep]], (c, p, ep)
            if F["fdump"] is not None and ep in dump_ep:
                u = F["cdef"][p].astype(np.int64) << su.RST_BITS
                for k in range(2):
                    want = F["fdump"][dump_ep.index(ep)][k][at:at + u.size].reshape(u.shape)
                    assert np.array_equal(flt[k] - u if flt[k] is not None else np.zeros_like(u), want), (c, p, ep, k)


@pytest.mark.parametrize("c", range(N_CASES))
def test_frame_filter_matches_reference(c):
    F = fixture_case(c)
    for r in range(len(F["ftype"])):
        out = su.filter_frame(F["cdef"], F["dbk"], F["w"], F["h"], F["bd"], F["ftype"][r], F["utype"][r], F["utaps"][r], F["usgr"][r])
        for p in range(3):
            assert np.array_equal(out[p], F["out"][r][p] if F["ftype"][r][p] else F["cdef"][p]), (c, r, p)
    assert (F["utype"][0] == 2).all() and np.array_equal(F["usgr"][0], F["sgrproj"])
    assert set(int(v) for v in F["utype"][1]) >= {2} and F["ftype"][2][0] == 0


def test_synthetic_solve():
    z = fixture()
    differs = [0, 0]
    for s, n, ep, xq, xqd, fd in zip(z["syn_sums"], z["syn_size"], z["syn_ep"], z["syn_xq"], z["syn_xqd"], z["syn_fused_differs"]):
        got = su.solve(s, int(n), int(ep))
        assert got[0] == [int(v) for v in xq] and got[1] == [int(v) for v in xqd]
        m = su.fused_mask(s, int(n), int(ep), got[0])
        assert m == int(fd)
        differs[0] += m & 1
        differs[1] += m >> 1
    assert min(differs) >= 5, "the rows would not notice one of the two fused forms of a * b - c * d"
    for p in range(2):
        assert (z["syn_xqd"][:, p] == su.PRJ_MIN[p]).any() and (z["syn_xqd"][:, p] == su.PRJ_MAX[p]).any()
    assert any((xq == 0).all() and (np.abs(s) > 0).any() for s, xq in zip(z["syn_sums"], z["syn_xq"])), "no row with Det < 1e-8"


def test_synthetic_walks_and_their_coverage():
    z = fixture()
    st = su.new_walk_stats()
    for coef, quant, ep, start, xqd, err, nt in zip(z["syn_walk_coef"], z["syn_walk_quant"], z["syn_walk_ep"], z["syn_walk_start"], z["syn_walk_xqd"],
                                                    z["syn_walk_err"], z["syn_walk_ntrials"]):
        T = walk_table(coef, quant)
        e, q, trace = su.walk(lambda x: int(T[x[0] - su.PRJ_MIN[0], x[1] - su.PRJ_MIN[1]]), [int(v) for v in start], int(ep), st)
        assert (e, q, len(trace)) == (int(err), [int(v) for v in xqd], int(nt))
        assert len(trace) <= su.max_walk_trials()
    assert all(st.values()), st


def synthetic_walk_stats():
    z = fixture()
    st = su.new_walk_stats()
    for coef, quant, ep, start in zip(z["syn_walk_coef"], z["syn_walk_quant"], z["syn_walk_ep"], z["syn_walk_start"]):
        T = walk_table(coef, quant)
        su.walk(lambda x: int(T[x[0] - su.PRJ_MIN[0], x[1] - su.PRJ_MIN[1]]), [int(v) for v in start], int(ep), st)
    return st


def test_fixture_covers_the_ground():
    """The rule: every arm of the issue's list is reached by a picture, or it is named in `unreached` and reached by a constructed case.
    Counted by the restatement on all eight pictures, whose run is the reference's trial by trial (test_search_matches_reference).  The
    constructed cases reach walk arms only, so an arm of the box filter, of the stripe rule, of the clip or the tie of sets must not be
    in `unreached` at all."""
    z = fixture()
    st_box, st_walk, st_flt = su.new_box_stats(), su.new_walk_stats(), su.new_filter_stats()
    tie = False
    for c in range(N_CASES):
        F = fixture_case(c)
        for p in range(3):
            for i, lim in enumerate(F["limits"][p]):
                u = F["base"][p] + i
                su.search_unit(F["cdef"][p], F["src"][p], lim, F["bd"], int(p > 0), st_box, st_walk)
                errs = [int(e) for e in F["detail"][u]["err"]]
                tie |= errs.count(min(errs)) > 1
        for r in range(3):
            su.filter_frame(F["cdef"], F["dbk"], F["w"], F["h"], F["bd"], F["ftype"][r], F["utype"][r], F["utaps"][r], F["usgr"][r], st_flt)
    reached = {**st_box, **{k: v for k, v in st_flt.items() if k != "neither"}, **st_walk, "best_ep_tie": int(tie)}
    unreached = [str(k) for k in z["unreached"]]
    assert sorted(k for k, v in reached.items() if not v) == sorted(unreached)
    syn = synthetic_walk_stats()
    for k in unreached:
        assert syn.get(k, 0) > 0, f"{k} is reached neither by a picture nor by a constructed case"


def test_walk_bound_is_the_documented_one():
    assert su.max_walk_trials() == 131


def _reference_available():
    import make_golden_lr as mg
    return mg.reference_available()


@pytest.mark.skipif(not _reference_available(), reason="needs the reference's sources and the oracle build (the build container); the fixture stands in")
def test_against_the_driver_directly(tmp_path):
    """the restatement against the driver itself, one 64x64 10-bit picture"""
    import make_golden_lr as mg
    import make_golden_lr_sgr as ms

    L = ms.build_driver(str(tmp_path))
    F = fixture_case(3)
    R = mg.Reference(L, F["w"], F["h"], F["bd"], F["cdef"], F["dbk"], F["src"])
    res = ms.reference_search(R, [len(v) for v in F["limits"]], True)
    R.close()
    for p in range(3):
        det, _, best = su.search_unit(F["cdef"][p], F["src"][p], F["limits"][p][0], F["bd"], int(p > 0))
        for k in det.dtype.names:
            assert np.array_equal(det[k], res[p]["detail"][0][k])
        assert list(best) == [int(v) for v in res[p]["sgrproj"][0][:3]]
