"""GPU: the Wiener loop-restoration entries bit-exact against the reference's fixture (tests/golden/lr.npz): statistics with every element
of M and H, the solve on the fixture's and on constructed M and H, the SSE of every recorded trial of one unit per case, the walk step
against the recorded traces and constructed error functions, the whole search (default step count, and three steps at a time resumed
until nothing is pending), the frame filter for every recorded assignment and fed from a search's device-side taps, the plane-subset
calls and every refusal.  Planes sit inside larger allocations with an odd guard of pattern samples that must come back untouched.
Everything is integer: every comparison is equality.  A tensor that torch fills is handed to an entry only after _ready()
(tests/lr_gpu_util.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import lr_util as lu  # noqa: E402
import svtav1_hip  # noqa: E402
from lr_gpu_util import DevCase, _dev, _ready  # noqa: E402
from test_lr_vs_ref import N_CASES, fixture, fixture_case, synthetic_error, taps_of, unit_traces  # noqa: E402

pytestmark = pytest.mark.gpu

INT64_MAX = lu.INT64_MAX


def _case(torch, F):
    return DevCase(torch, F, svtav1_hip.lr_workspace_bytes(F["base"][3]))


@pytest.mark.parametrize("c", range(N_CASES))
def test_stats_match_fixture(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = _case(torch, F)
    n = D.n
    d_M = torch.full((n, 49), -1, dtype=torch.int64, device="cuda:0")
    d_H = torch.full((n, 49 * 49), -1, dtype=torch.int64, device="cuda:0")
    d_avg = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    d_none = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
    _ready(torch)
    hip_ctx.av1_wiener_stats_dev(D.pic, 0, 3, d_M.data_ptr(), d_H.data_ptr(), d_avg.data_ptr(), d_none.data_ptr(), D.work.data_ptr(), bit_depth=F["bd"])
    hip_ctx.synchronize()
    M, H = d_M.cpu().numpy(), d_H.cpu().numpy()
    for u in range(n):
        k = F["win"][u] ** 2
        assert np.array_equal(M[u, :k], F["M"][u][:k]) and np.array_equal(H[u, :k * k], F["H"][u][:k * k]), (c, u)
        assert (M[u, k:] == -1).all() and (H[u, k * k:] == -1).all(), (c, u)
    assert np.array_equal(d_avg.cpu().numpy(), F["avg"]) and np.array_equal(d_none.cpu().numpy(), F["sse"][:, 0])
    assert D.inputs_untouched()


def test_solve_matches_fixture_and_constructed(hip_ctx):
    torch = pytest.importorskip("torch")
    z = fixture()
    Ms, Hs, wins, starts, rejs = [], [], [], [], []
    for c in range(N_CASES):
        F = fixture_case(c)
        Ms += list(F["M"])
        Hs += list(F["H"])
        wins += list(F["win"])
        starts += list(F["start"])
        rejs += list(F["rejected"])
    Ms += list(z["syn_M"])
    Hs += list(z["syn_H"])
    wins += [int(w) for w in z["syn_win"]]
    starts += list(z["syn_start"])
    rejs += list(z["syn_rejected"])
    order = sorted(range(len(wins)), key=lambda i: -wins[i])   # the luma units first: one call per window size
    n7 = sum(1 for w in wins if w == 7)
    d_M, d_H = _dev(torch, np.array([Ms[i] for i in order], np.int64)), _dev(torch, np.array([Hs[i] for i in order], np.int64))
    d_taps = torch.full((len(order), 16), -1, dtype=torch.int16, device="cuda:0")
    d_rej = torch.full((len(order),), -1, dtype=torch.int32, device="cuda:0")
    _ready(torch)
    hip_ctx.wiener_solve_dev(d_M.data_ptr(), d_H.data_ptr(), 0, n7, 7, d_taps.data_ptr(), d_rej.data_ptr())
    hip_ctx.wiener_solve_dev(d_M.data_ptr(), d_H.data_ptr(), n7, len(order), 5, d_taps.data_ptr(), d_rej.data_ptr())
    hip_ctx.synchronize()
    assert np.array_equal(d_taps.cpu().numpy(), np.array([starts[i] for i in order], np.int16))
    assert np.array_equal(d_rej.cpu().numpy(), np.array([rejs[i] for i in order], np.int32))
    assert any(rejs) and not all(rejs)


@pytest.mark.parametrize("c", range(N_CASES))
def test_trial_sse_matches_every_recorded_trial_of_a_unit(hip_ctx, c):
    """the unit with the most trials; the other units carry default taps or are skipped"""
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = _case(torch, F)
    traces = unit_traces(F)
    u = int(np.argmax(F["n_trials"]))
    p = F["plane"][u]
    taps = np.zeros((D.n, 16), np.int16)
    skip = np.ones(D.n, np.uint8)
    skip[u] = 0
    d_skip = _dev(torch, skip)
    d_sse = torch.full((D.n,), -1, dtype=torch.int64, device="cuda:0")
    _ready(torch)
    got = []
    for (t, _) in traces[u]:
        taps[u] = t
        d_t = _dev(torch, taps)
        hip_ctx.av1_wiener_trial_sse_dev(D.pic, p, p + 1, d_t.data_ptr(), d_sse.data_ptr(), d_skip.data_ptr(), bit_depth=F["bd"])
        hip_ctx.synchronize()
        got.append(d_sse.cpu().numpy().copy())
    assert [int(g[u]) for g in got] == [e for (_, e) in traces[u]], (c, u)
    for g in got:   # skipped units of the plane read 0, units of other planes are not written
        for v in range(D.n):
            if v != u:
                assert g[v] == (0 if F["plane"][v] == p else -1)
    # all units of all planes at once, nothing skipped: the first recorded trial of each (the start taps)
    first = np.array([traces[v][0][0] if traces[v] else F["start"][v] for v in range(D.n)], np.int16)
    d_first = _dev(torch, first)
    hip_ctx.av1_wiener_trial_sse_dev(D.pic, 0, 3, d_first.data_ptr(), d_sse.data_ptr(), None, bit_depth=F["bd"])
    hip_ctx.synchronize()
    g = d_sse.cpu().numpy()
    for v in range(D.n):
        if traces[v]:
            assert int(g[v]) == traces[v][0][1], (c, v)
    assert D.inputs_untouched()


def _run_walks(torch, hip_ctx, jobs):
    """jobs: [(start taps[16], win, rejected, error function of (vfilter, hfilter))] -> per job (err, taps, trials asked [(taps, sse)])"""
    order = sorted(range(len(jobs)), key=lambda i: -jobs[i][1])
    n, n7 = len(jobs), sum(1 for j in jobs if j[1] == 7)
    d_taps = _dev(torch, np.array([jobs[i][0] for i in order], np.int16))
    d_rej = _dev(torch, np.array([jobs[i][2] for i in order], np.int32))
    d_state = torch.zeros(n * 56, dtype=torch.uint8, device="cuda:0")
    d_pending = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    _ready(torch)
    hip_ctx.wiener_walk_init_dev(d_state.data_ptr(), d_taps.data_ptr(), d_rej.data_ptr(), 0, n7, 7)
    hip_ctx.wiener_walk_init_dev(d_state.data_ptr(), d_taps.data_ptr(), d_rej.data_ptr(), n7, n, 5)
    asked = [[] for _ in range(n)]
    for _ in range(svtav1_hip.wiener_walk_max_trials(7) + 1):
        hip_ctx.synchronize()
        st = d_state.cpu().numpy().view(svtav1_hip.WIENER_WALK_STATE_DTYPE)
        if st["done"].all():
            break
        sse = np.zeros(n, np.int64)
        for k, i in enumerate(order):
            if not st["done"][k]:
                t = [int(v) for v in st["taps"][k]]
                sse[k] = jobs[i][3](t[:8], t[8:])
                asked[i].append((t, int(sse[k])))
        d_e = _dev(torch, sse)
        hip_ctx.wiener_walk_step_dev(d_state.data_ptr(), d_e.data_ptr(), 0, n, d_pending.data_ptr())
        hip_ctx.synchronize()
        assert int(d_pending.cpu()[0]) == int((d_state.cpu().numpy().view(svtav1_hip.WIENER_WALK_STATE_DTYPE)["done"] == 0).sum())
    st = d_state.cpu().numpy().view(svtav1_hip.WIENER_WALK_STATE_DTYPE)
    assert st["done"].all(), "a walk is longer than svthip_wiener_walk_max_trials"
    out = [None] * n
    for k, i in enumerate(order):
        assert st["n_trials"][k] == len(asked[i])
        out[i] = (int(st["err"][k]), [int(v) for v in st["taps"][k]], asked[i])
    return out


def test_walk_step_follows_the_recorded_traces(hip_ctx):
    torch = pytest.importorskip("torch")
    jobs, want = [], []
    for c in range(N_CASES):
        F = fixture_case(c)
        for u, tr in enumerate(unit_traces(F)):
            table = dict((tuple(k), e) for k, e in tr)
            jobs.append((F["start"][u].tolist(), F["win"][u], int(F["rejected"][u]), lambda a, b, t=table: t[tuple(a) + tuple(b)]))
            want.append((int(F["sse"][u][1]), F["final"][u].tolist(), tr))
    got = _run_walks(torch, hip_ctx, jobs)
    for g, w in zip(got, want):
        assert g == w


def test_walk_step_on_constructed_error_functions(hip_ctx):
    """ties, taps stopped by their range, long runs at step 4, and a rejected unit that never asks for a trial"""
    torch = pytest.importorskip("torch")
    z = fixture()
    jobs, want = [], []
    for coef, start, win, quant, fin, ntr, err in zip(z["syn_walk_coef"], z["syn_walk_start"], z["syn_walk_win"], z["syn_walk_quant"],
                                                      z["syn_walk_final"], z["syn_walk_ntrials"], z["syn_walk_err"]):
        vf, hf = taps_of(start)
        fn = synthetic_error(coef, quant)
        jobs.append((vf + hf, int(win), 0, fn))
        want.append((int(err), fin.tolist(), lu.walk(fn, vf, hf, int(win))[3]))
    jobs.append((jobs[0][0], 7, 1, jobs[0][3]))
    want.append((INT64_MAX, jobs[0][0], []))
    got = _run_walks(torch, hip_ctx, jobs)
    for g, w in zip(got, want):
        assert g == w
    assert [len(g[2]) for g in got[:-1]] == [int(v) for v in z["syn_walk_ntrials"]]


def _search(torch, hip_ctx, D, F, ps, pe, n_steps):
    n = D.n
    d_sse = torch.full((n, 2), -1, dtype=torch.int64, device="cuda:0")
    d_taps = torch.full((n, 16), -1, dtype=torch.int16, device="cuda:0")
    d_ntr = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    d_pending = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    _ready(torch)
    args = (D.pic, ps, pe, D.work.data_ptr(), d_sse.data_ptr(), d_taps.data_ptr(), d_ntr.data_ptr(), d_pending.data_ptr())
    hip_ctx.av1_search_wiener_dev(*args, n_steps=n_steps, bit_depth=F["bd"])
    hip_ctx.synchronize()
    calls = 1
    while int(d_pending.cpu()[0]) != 0:
        assert n_steps and calls * n_steps <= svtav1_hip.wiener_walk_max_trials(7), "the search does not end"
        hip_ctx.av1_search_wiener_dev(*args, n_steps=n_steps, resume=True, bit_depth=F["bd"])
        hip_ctx.synchronize()
        calls += 1
    return d_sse, d_taps, d_ntr, calls


@pytest.mark.parametrize("c", range(N_CASES))
def test_search_matches_reference_and_feeds_the_filter(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = _case(torch, F)
    for n_steps in (0, 3):
        d_sse, d_taps, d_ntr, calls = _search(torch, hip_ctx, D, F, 0, 3, n_steps)
        assert np.array_equal(d_sse.cpu().numpy(), F["sse"]), (c, n_steps)
        assert np.array_equal(d_taps.cpu().numpy(), F["final"]), (c, n_steps)
        assert np.array_equal(d_ntr.cpu().numpy(), F["n_trials"]), (c, n_steps)
        assert calls == (1 if n_steps == 0 else max(1, -(-int(F["n_trials"].max()) // 3))), (c, n_steps, calls)
    assert D.inputs_untouched()
    # the taps stay on the device: run 0 of the fixture is the reference's frame filter with the search's taps, all units Wiener
    if not F["rejected"].any():
        assert np.array_equal(F["utaps"][0], F["final"])
        d_type = _dev(torch, F["utype"][0])
        hip_ctx.av1_loop_restoration_filter_frame_dev(D.pic, D.out.ptr, D.out.stride, 0, 3, d_type.data_ptr(), d_taps.data_ptr(), bit_depth=F["bd"])
        hip_ctx.synchronize()
        got, guard_ok = D.out.planes()
        assert guard_ok and all(np.array_equal(g, o) for g, o in zip(got, F["out"][0])), c


@pytest.mark.parametrize("c", range(N_CASES))
def test_frame_filter_matches_fixture(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    for r in range(len(F["ftype"])):
        D = _case(torch, F)
        d_type, d_taps = _dev(torch, F["utype"][r]), _dev(torch, F["utaps"][r])
        planes = [p for p in range(3) if F["ftype"][r][p]]
        hip_ctx.av1_loop_restoration_filter_frame_dev(D.pic, D.out.ptr, D.out.stride, planes[0], planes[-1] + 1, d_type.data_ptr(), d_taps.data_ptr(),
                                                      bit_depth=F["bd"])
        hip_ctx.synchronize()
        got, guard_ok = D.out.planes()
        for p in range(3):
            want = F["out"][r][p] if F["ftype"][r][p] else np.full_like(F["cdef"][p], 7)   # a plane outside the call is not written
            assert np.array_equal(got[p], want), (c, r, p)
        assert guard_ok and D.inputs_untouched(), (c, r)
        assert hip_ctx.inter_pred_refused() == 0


def test_plane_subset_calls(hip_ctx):
    """a chroma-only search and a luma-only filter with null entries for the other planes"""
    torch = pytest.importorskip("torch")
    F = fixture_case(1)
    D = _case(torch, F)
    b = F["base"]
    cb = svtav1_hip.make_lr_picture(F["w"], F["h"], [None, D.cdef.ptr[1], None], D.cdef.stride, [None, D.dbk.ptr[1], None], D.dbk.stride,
                                    [None, D.src.ptr[1], None], D.src.stride)
    keep = D.pic
    D.pic = cb
    d_sse, d_taps, d_ntr, _ = _search(torch, hip_ctx, D, F, 1, 2, 0)
    D.pic = keep
    sse, taps, ntr = d_sse.cpu().numpy(), d_taps.cpu().numpy(), d_ntr.cpu().numpy()
    assert np.array_equal(sse[b[1]:b[2]], F["sse"][b[1]:b[2]]) and np.array_equal(taps[b[1]:b[2]], F["final"][b[1]:b[2]])
    assert np.array_equal(ntr[b[1]:b[2]], F["n_trials"][b[1]:b[2]])
    assert (sse[:b[1]] == -1).all() and (sse[b[2]:] == -1).all() and (ntr[:b[1]] == -1).all() and (ntr[b[2]:] == -1).all()
    luma = svtav1_hip.make_lr_picture(F["w"], F["h"], [D.cdef.ptr[0], None, None], D.cdef.stride, [D.dbk.ptr[0], None, None], D.dbk.stride)
    d_type, d_t = _dev(torch, F["utype"][1]), _dev(torch, F["utaps"][1])
    hip_ctx.av1_loop_restoration_filter_frame_dev(luma, [D.out.ptr[0], None, None], D.out.stride, 0, 1, d_type.data_ptr(), d_t.data_ptr(), bit_depth=F["bd"])
    hip_ctx.synchronize()
    got, guard_ok = D.out.planes()
    assert guard_ok and np.array_equal(got[0], F["out"][1][0]) and (got[1] == 7).all() and (got[2] == 7).all()
    with pytest.raises(svtav1_hip.SvtHipError):
        hip_ctx.av1_loop_restoration_filter_frame_dev(luma, [D.out.ptr[0], None, None], D.out.stride, 0, 2, d_type.data_ptr(), d_t.data_ptr())


def test_sgrproj_unit_is_refused_on_the_device(hip_ctx):
    torch = pytest.importorskip("torch")
    F = fixture_case(1)
    D = _case(torch, F)
    types = F["utype"][0].copy()
    types[1] = svtav1_hip.RESTORE_SGRPROJ
    assert hip_ctx.inter_pred_refused() == 0
    d_type, d_taps = _dev(torch, types), _dev(torch, F["utaps"][0])   # kept alive: a freed temporary's memory is handed to the next one
    hip_ctx.av1_loop_restoration_filter_frame_dev(D.pic, D.out.ptr, D.out.stride, 0, 3, d_type.data_ptr(), d_taps.data_ptr())
    hip_ctx.synchronize()
    with pytest.raises(svtav1_hip.SvtHipError, match=r": 1 PU\(s\) or unit\(s\) refused"):
        hip_ctx.inter_pred_refused()
    assert hip_ctx.inter_pred_refused() == 0   # the query clears the count
    got, guard_ok = D.out.planes()
    h0, h1, v0, v1 = (int(v) for v in F["limits"][1])
    want = F["out"][0][0].copy()
    want[v0:v1, h0:h1] = 7                     # nothing of the refused unit is written
    assert guard_ok and np.array_equal(got[0], want) and np.array_equal(got[1], F["out"][0][1]) and np.array_equal(got[2], F["out"][0][2])


def test_refusals(hip_ctx):
    """refused on the host, before any launch: nothing is written"""
    torch = pytest.importorskip("torch")
    F = fixture_case(0)
    D = _case(torch, F)
    n = D.n
    d64 = torch.full((n * 49 * 49,), -1, dtype=torch.int64, device="cuda:0")
    d32 = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    d16 = torch.full((n, 16), -1, dtype=torch.int16, device="cuda:0")
    _ready(torch)
    d8 = _dev(torch, F["utype"][0])
    w, h = F["w"], F["h"]
    mk = lambda **k: svtav1_hip.make_lr_picture(k.get("w", w), k.get("h", h), k.get("cdef", D.cdef.ptr), D.cdef.stride, D.dbk.ptr,  # noqa: E731
                                                k.get("dstride", D.dbk.stride), D.src.ptr, D.src.stride, k.get("unit"))
    odd, unit96, no_cb, narrow = mk(w=w - 4), mk(unit=(128, 96, 64)), mk(cdef=[D.cdef.ptr[0], None, D.cdef.ptr[2]]), mk(dstride=[8, 8, 8])
    stats = lambda pic, ps=0, pe=3, bd=F["bd"], work=D.work.data_ptr(): hip_ctx.av1_wiener_stats_dev(  # noqa: E731
        pic, ps, pe, d64.data_ptr(), d64.data_ptr(), d32.data_ptr(), d64.data_ptr(), work, bit_depth=bd)
    trial = lambda pic, ps=0, pe=3, taps=d16.data_ptr(): hip_ctx.av1_wiener_trial_sse_dev(pic, ps, pe, taps, d64.data_ptr(), None, bit_depth=F["bd"])  # noqa: E731
    search = lambda pic, ps=0, pe=3, bd=F["bd"], work=D.work.data_ptr(): hip_ctx.av1_search_wiener_dev(  # noqa: E731
        pic, ps, pe, work, d64.data_ptr(), d16.data_ptr(), d32.data_ptr(), d32.data_ptr(), bit_depth=bd)
    frame = lambda pic, ps=0, pe=3, out=D.out.ptr, types=d8.data_ptr(), bd=F["bd"]: hip_ctx.av1_loop_restoration_filter_frame_dev(  # noqa: E731
        pic, out, D.out.stride, ps, pe, types, d16.data_ptr(), bit_depth=bd)
    calls = []
    for f in (stats, trial, search, frame):
        calls += [lambda f=f: f(odd), lambda f=f: f(unit96), lambda f=f: f(no_cb), lambda f=f: f(narrow), lambda f=f: f(None),
                  lambda f=f: f(D.pic, 1, 1), lambda f=f: f(D.pic, 2, 1), lambda f=f: f(D.pic, 0, 4)]
    calls += [lambda: stats(D.pic, bd=12), lambda: search(D.pic, bd=12), lambda: frame(D.pic, bd=12), lambda: stats(D.pic, work=None),
              lambda: search(D.pic, work=None), lambda: trial(D.pic, taps=None), lambda: frame(D.pic, types=None),
              lambda: frame(D.pic, out=[D.out.ptr[0], None, D.out.ptr[2]]),
              lambda: hip_ctx.wiener_solve_dev(d64.data_ptr(), d64.data_ptr(), 0, 1, 6, d16.data_ptr(), d32.data_ptr()),
              lambda: hip_ctx.wiener_solve_dev(None, d64.data_ptr(), 0, 1, 7, d16.data_ptr(), d32.data_ptr()),
              lambda: hip_ctx.wiener_solve_dev(d64.data_ptr(), d64.data_ptr(), 2, 1, 7, d16.data_ptr(), d32.data_ptr()),
              lambda: hip_ctx.wiener_walk_init_dev(None, d16.data_ptr(), None, 0, 1, 7),
              lambda: hip_ctx.wiener_walk_init_dev(d64.data_ptr(), d16.data_ptr(), None, 0, 1, 3),
              lambda: hip_ctx.wiener_walk_step_dev(d64.data_ptr(), None, 0, 1), lambda: hip_ctx.wiener_walk_step_dev(None, d64.data_ptr(), 0, 1)]
    for i, call in enumerate(calls):
        with pytest.raises(svtav1_hip.SvtHipError):
            call()
    hip_ctx.synchronize()
    got, guard_ok = D.out.planes()
    assert guard_ok and all((g == 7).all() for g in got) and D.inputs_untouched()
    assert bool((d64 == -1).all()) and bool((d32 == -1).all()) and bool((d16 == -1).all())
    # the planes of a call are the only ones checked: a luma call on the picture without Cb is fine
    stats(no_cb, 0, 1)
    hip_ctx.synchronize()
    assert int(d32.cpu()[0]) == F["avg"][0]
