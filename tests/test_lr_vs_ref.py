"""CPU: the numpy restatement of the Wiener restoration search and frame filter (tests/lr_util.py) equals the reference's own run recorded
in tests/golden/lr.npz (tests/golden/make_golden_lr.py), entry by entry, the trial trace included; the fixture covers the ground the
feature's rules cover, counted on the reference's recorded run.  Arms the pictures do not reach are named in the fixture's `unreached`
(today: a tie in the walk, a unit rejected by compute_score) and are covered by constructed cases answered by the restatement alone."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import lr_util as lu  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "lr.npz")
N_CASES = 7


@functools.lru_cache(maxsize=None)
def fixture():
    assert os.path.exists(FIXTURE), "tests/golden/lr.npz is missing (python tests/golden/make_golden_lr.py in the build container)"
    return dict(np.load(FIXTURE))


@functools.lru_cache(maxsize=None)
def fixture_case(c):
    return lu.load_case(fixture(), c)


def unit_traces(F):
    """per unit the recorded trials [(taps[16], sse)]"""
    at, out = 0, []
    for n in F["n_trials"]:
        out.append([([int(t) for t in F["trace_taps"][i]], int(F["trace_sse"][i])) for i in range(at, at + int(n))])
        at += int(n)
    return out


def synthetic_error(coef, quant):
    def err(vf, hf):
        t = [int(v) for v in vf[:3]] + [int(v) for v in hf[:3]]
        e = sum(int(c[0]) * (t[i] - int(c[1])) ** 2 + int(c[2]) * abs(t[i] - int(c[1])) for i, c in enumerate(coef))
        return 1000000 + e // int(quant) * int(quant)
    return err


def taps_of(start6):
    v, h = [int(t) for t in start6[:3]], [int(t) for t in start6[3:]]
    return (v + [-2 * sum(v)] + v[::-1] + [0]), (h + [-2 * sum(h)] + h[::-1] + [0])


def test_fixture_has_the_cases():
    z = fixture()
    assert [tuple(r) for r in z["case"]] == [(64, 64, 8), (200, 136, 8), (136, 200, 8), (392, 264, 8), (64, 64, 10), (200, 136, 10), (136, 200, 10)]
    assert len(z["syn_walk_win"]) and len(z["syn_win"])


@pytest.mark.parametrize("c", range(N_CASES))
def test_geometry_matches_reference(c):
    F = fixture_case(c)
    planes, base = lu.picture_units(F["w"], F["h"])
    assert base == F["base"] and tuple(F["unit_size"]) == lu.unit_sizes(F["w"], F["h"])
    assert np.array_equal(np.concatenate([p[0] for p in planes]), F["limits"])


@pytest.mark.parametrize("c", range(N_CASES))
def test_stats_and_solve_match_reference(c):
    F = fixture_case(c)
    for u, lim in enumerate(F["limits"]):
        p, win = F["plane"][u], F["win"][u]
        M, H, avg = lu.compute_stats(F["cdef"][p], F["src"][p], lim, win, F["bd"])
        n = win * win
        assert avg == F["avg"][u] and np.array_equal(M, F["M"][u][:n]) and np.array_equal(H.reshape(-1), F["H"][u][:n * n]), (c, u)
        assert lu.unit_sse(F["src"][p], F["cdef"][p], lim) == F["sse"][u][0], (c, u)
        vf, hf, rej = lu.solve(F["M"][u], F["H"][u], win)
        assert vf + hf == F["start"][u].tolist() and int(rej) == F["rejected"][u], (c, u)


def test_solver_on_constructed_statistics():
    z = fixture()
    for M, H, win, start, rej in zip(z["syn_M"], z["syn_H"], z["syn_win"], z["syn_start"], z["syn_rejected"]):
        vf, hf, r = lu.solve(M, H, int(win))
        assert vf + hf == start.tolist() and int(r) == rej
    assert z["syn_rejected"].any() and not z["syn_rejected"].all()


@pytest.mark.parametrize("c", range(N_CASES))
def test_search_trace_matches_reference(c):
    """every trial the reference ran: the restatement's walk asks for the same taps in the same order and its unit filter gives the same SSE"""
    F = fixture_case(c)
    traces = unit_traces(F)
    for u, lim in enumerate(F["limits"]):
        p, win = F["plane"][u], F["win"][u]
        if F["rejected"][u]:
            assert F["sse"][u][1] == lu.INT64_MAX and F["n_trials"][u] == 0
            continue
        fn = lambda a, b: lu.trial_sse(F["cdef"][p], F["dbk"][p], F["src"][p], lim, a, b, F["bd"], int(p > 0))  # noqa: E731
        err, vf, hf, trace = lu.walk(fn, F["start"][u][:8].tolist(), F["start"][u][8:].tolist(), win)
        assert trace == traces[u], (c, u)
        assert err == F["sse"][u][1] and vf + hf == F["final"][u].tolist() and len(trace) <= lu.max_walk_trials(win), (c, u)
        # the state machine the device runs is the same walk
        assert lu.walk_by_steps(lambda a, b, t=dict((tuple(k), e) for k, e in trace): t[tuple(a) + tuple(b)], F["start"][u][:8].tolist(),
                                F["start"][u][8:].tolist(), win) == (err, vf, hf, trace), (c, u)


@pytest.mark.parametrize("c", range(N_CASES))
def test_frame_filter_matches_reference(c):
    F = fixture_case(c)
    for r in range(len(F["ftype"])):
        got = lu.filter_frame(F["cdef"], F["dbk"], F["w"], F["h"], F["bd"], F["ftype"][r], F["utype"][r], F["utaps"][r])
        for p in range(3):
            want = F["out"][r][p] if F["ftype"][r][p] else F["cdef"][p]
            assert np.array_equal(got[p], want), (c, r, p)
    assert len(F["ftype"]) >= 3 and (F["ftype"] == 0).any() and (F["utype"] == 0).any() and (F["utype"] == 1).all(axis=1).any()


def test_walk_on_constructed_error_functions():
    z = fixture()
    st = lu.new_walk_stats()
    for coef, start, win, quant, fin, ntr, err in zip(z["syn_walk_coef"], z["syn_walk_start"], z["syn_walk_win"], z["syn_walk_quant"],
                                                      z["syn_walk_final"], z["syn_walk_ntrials"], z["syn_walk_err"]):
        vf, hf = taps_of(start)
        fn = synthetic_error(coef, quant)
        a = lu.walk(fn, vf, hf, int(win), st)
        assert a == lu.walk_by_steps(fn, vf, hf, int(win))
        assert (a[0], a[1] + a[2], len(a[3])) == (int(err), fin.tolist(), int(ntr)) and ntr <= lu.max_walk_trials(int(win))
    assert all(st.values()), st


def test_fixture_covers_the_ground():
    """counted on the reference's own recorded run: its trials (taps and SSE as recorded) and its frame-filter runs"""
    z = fixture()
    st_f, st_w = lu.new_filter_stats(), lu.new_walk_stats()
    geo = {"early_start": False, "early_end": False, "wide_remainder": False}
    rejected = False
    for c in range(N_CASES):
        F = fixture_case(c)
        traces = unit_traces(F)
        rejected |= bool(F["rejected"].any())
        for u, lim in enumerate(F["limits"]):
            p, ss = F["plane"][u], int(F["plane"][u] > 0)
            ph, unit, off = F["h"] >> ss, int(F["unit_size"][p]), 8 >> ss
            h0, h1, v0, v1 = (int(v) for v in lim)
            geo["early_start"] |= v0 > 0 and (v0 + off) % unit == 0
            geo["early_end"] |= v1 < ph
            geo["wide_remainder"] |= (h1 - h0) > unit or (v1 - v0) > unit
            if not traces[u]:
                continue
            for taps, _ in traces[u][:3]:
                lu.filter_unit(F["cdef"][p], F["dbk"][p], lim, taps[:8], taps[8:], F["bd"], ss, st_f)
            table = dict((tuple(k), e) for k, e in traces[u])
            lu.walk(lambda a, b: table[tuple(a) + tuple(b)], traces[u][0][0][:8], traces[u][0][0][8:], F["win"][u], st_w)
        for r in range(len(F["ftype"])):
            lu.filter_frame(F["cdef"], F["dbk"], F["w"], F["h"], F["bd"], F["ftype"][r], F["utype"][r], F["utaps"][r], st=st_f)
    reached = {k: bool(v) for k, v in {**st_f, **st_w, **geo, "rejected": rejected}.items() if k != "neither"}
    unreached = set(str(k) for k in z["unreached"])
    assert unreached == {k for k, v in reached.items() if not v}, (reached, unreached)
    assert unreached <= {"tie", "rejected"}, unreached
    # what the pictures do not reach, the constructed cases do
    if "tie" in unreached:
        st = lu.new_walk_stats()
        for coef, start, win, quant in zip(z["syn_walk_coef"], z["syn_walk_start"], z["syn_walk_win"], z["syn_walk_quant"]):
            lu.walk(synthetic_error(coef, quant), *taps_of(start), int(win), st)
        assert st["tie"]
    if "rejected" in unreached:
        assert z["syn_rejected"].any()
