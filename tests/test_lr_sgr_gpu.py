"""GPU: the self-guided loop-restoration entries bit-exact against the reference's fixture (tests/golden/lr_sgr.npz): the box filter over a
plane (the samples of the 64x64 pictures at one set per arm, the sums of all sets of a 200x136 picture), the solve on the fixture's and on
constructed sums (rows that a fused multiply-add would change among them), the walk on constructed error tables, the whole search with
every record of every (unit, set), the SSE trial, and the frame filter for every recorded run and fed from a search's device-side result.
Planes sit inside larger allocations with an odd guard of pattern samples that must come back untouched.  Every comparison is equality.
A tensor that torch fills is handed to an entry only after _ready() (tests/lr_gpu_util.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import lr_sgr_util as su  # noqa: E402
import svtav1_hip  # noqa: E402
from lr_gpu_util import DevCase, _dev, _ready  # noqa: E402
from test_lr_sgr_vs_ref import N_CASES, fixture, fixture_case, walk_table  # noqa: E402

pytestmark = pytest.mark.gpu


def _case(torch, F):
    return DevCase(torch, F, svtav1_hip.sgrproj_workspace_bytes(F["w"], F["h"]))


def _plane_flt(torch, hip_ctx, D, p, ep):
    """flt0, flt1 of plane p inside guarded int32 allocations (pitch = width + 5); a plane of radius 0 gets a null pointer"""
    ph, pw = D.F["cdef"][p].shape
    pitch, out = pw + 5, []
    bufs = [torch.full((ph + 2, pitch), -7, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    ptr = [bufs[k].data_ptr() + pitch * 4 if su.SGR_R[ep][k] else None for k in range(2)]
    _ready(torch)
    hip_ctx.av1_selfguided_restoration_dev(D.pic, p, ep, ptr[0], ptr[1], pitch, bit_depth=D.bd)
    hip_ctx.synchronize()
    for k in range(2):
        b = bufs[k].cpu().numpy()
        assert (b[0] == -7).all() and (b[-1] == -7).all() and (b[:, pw:] == -7).all(), "the plane entry wrote outside the plane"
        out.append(b[1:-1, :pw].astype(np.int64) if su.SGR_R[ep][k] else None)
        if not su.SGR_R[ep][k]:
            assert (b == -7).all()
    return out


@pytest.mark.parametrize("c", (0, 3, 6, 7))
def test_plane_entry_matches_the_samples_of_three_sets(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = _case(torch, F)
    for e, ep in enumerate(int(v) for v in fixture()["dump_ep"]):
        for p in range(3):
            at = sum(F["cdef"][q].size for q in range(p))
            u = F["cdef"][p].astype(np.int64) << su.RST_BITS
            got = _plane_flt(torch, hip_ctx, D, p, ep)
            for k in range(2):
                if got[k] is not None:
                    assert np.array_equal(got[k] - u, F["fdump"][e][k][at:at + u.size].reshape(u.shape)), (c, ep, p, k)
    assert D.inputs_untouched()


@pytest.mark.parametrize("c", (1, 4))
def test_plane_entry_matches_the_sums_of_every_set(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = _case(torch, F)
    for p in range(3):
        for ep in range(16):
            got = _plane_flt(torch, hip_ctx, D, p, ep)
            mine = [v for k in range(2) for v in ((int(got[k].sum()), int((got[k] * got[k]).sum())) if got[k] is not None else (0, 0))]
            assert mine == [int(v) for v in F["fsums"][p][ep]], (c, p, ep)
    assert D.inputs_untouched()


def test_solve_matches_fixture_and_constructed(hip_ctx):
    torch = pytest.importorskip("torch")
    z = fixture()
    sums, size, ep, xq, xqd = [z["syn_sums"]], [z["syn_size"]], [z["syn_ep"]], [z["syn_xq"]], [z["syn_xqd"]]
    for c in range(N_CASES):
        F = fixture_case(c)
        for p in range(3):
            for i, lim in enumerate(F["limits"][p]):
                d = F["detail"][F["base"][p] + i]
                sums.append(d["sums"]), xq.append(d["exq"]), xqd.append(d["start_xqd"])
                size.append(np.full(16, (int(lim[1]) - int(lim[0])) * (int(lim[3]) - int(lim[2])), np.int32)), ep.append(np.arange(16, dtype=np.int32))
    sums, size, ep = np.concatenate(sums).astype(np.int64), np.concatenate(size).astype(np.int32), np.concatenate(ep).astype(np.int32)
    n = len(ep)
    d_s, d_n, d_e = _dev(torch, sums), _dev(torch, size), _dev(torch, ep)
    d_xq = torch.full((n + 1, 2), -7, dtype=torch.int32, device="cuda:0")
    d_xqd = torch.full((n + 1, 2), -7, dtype=torch.int32, device="cuda:0")
    _ready(torch)
    hip_ctx.sgrproj_solve_dev(d_s.data_ptr(), d_n.data_ptr(), d_e.data_ptr(), n, d_xq.data_ptr(), d_xqd.data_ptr())
    hip_ctx.synchronize()
    gq, gd = d_xq.cpu().numpy(), d_xqd.cpu().numpy()
    assert np.array_equal(gq[:n], np.concatenate(xq)) and np.array_equal(gd[:n], np.concatenate(xqd))
    assert (gq[n] == -7).all() and (gd[n] == -7).all()
    assert int((z["syn_fused_differs"] & 1).sum()) >= 5 and int((z["syn_fused_differs"] >> 1).sum()) >= 5


def test_walk_on_constructed_tables(hip_ctx):
    torch = pytest.importorskip("torch")
    z = fixture()
    n = len(z["syn_walk_ep"])
    tables = np.array([walk_table(c, q) for c, q in zip(z["syn_walk_coef"], z["syn_walk_quant"])], np.int64)
    assert tables.shape == (n, 128, 128)
    d_t, d_e, d_s = _dev(torch, tables), _dev(torch, z["syn_walk_ep"].astype(np.int32)), _dev(torch, z["syn_walk_start"].astype(np.int32))
    d_x = torch.full((n + 1, 2), -7, dtype=torch.int32, device="cuda:0")
    d_err = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda:0")
    d_nt = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda:0")
    _ready(torch)
    hip_ctx.sgrproj_walk_table_dev(d_t.data_ptr(), d_e.data_ptr(), d_s.data_ptr(), n, d_x.data_ptr(), d_err.data_ptr(), d_nt.data_ptr())
    hip_ctx.synchronize()
    x, e, nt = d_x.cpu().numpy(), d_err.cpu().numpy(), d_nt.cpu().numpy()
    assert np.array_equal(x[:n], z["syn_walk_xqd"]) and np.array_equal(e[:n], z["syn_walk_err"]) and np.array_equal(nt[:n], z["syn_walk_ntrials"])
    assert (x[n] == -7).all() and e[n] == -7 and nt[n] == -7
    assert int(nt[:n].max()) <= svtav1_hip.sgrproj_walk_max_trials()


def _search(torch, hip_ctx, D, ps, pe, pic=None, detail=True):
    d_sgr = torch.full((D.n, 4), -1, dtype=torch.int32, device="cuda:0")
    d_sse = torch.full((D.n,), -1, dtype=torch.int64, device="cuda:0")
    d_det = torch.full((D.n * 16 * 80,), 0xEE, dtype=torch.uint8, device="cuda:0")
    _ready(torch)
    hip_ctx.av1_search_sgrproj_dev(pic or D.pic, ps, pe, D.work.data_ptr(), d_sgr.data_ptr(), d_sse.data_ptr(), d_det.data_ptr() if detail else None,
                                   bit_depth=D.bd)
    return d_sgr, d_sse, d_det


@pytest.mark.parametrize("c", range(N_CASES))
def test_search_matches_fixture_with_every_record(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = _case(torch, F)
    d_sgr, d_sse, d_det = _search(torch, hip_ctx, D, 0, 3)
    hip_ctx.synchronize()
    det = d_det.cpu().numpy().view(svtav1_hip.SGRPROJ_DETAIL_DTYPE).reshape(D.n, 16)
    for k in det.dtype.names:
        assert np.array_equal(det[k], F["detail"][k]), (c, k)
    assert np.array_equal(d_sgr.cpu().numpy(), F["sgrproj"]) and np.array_equal(d_sse.cpu().numpy(), F["sse"])
    assert int(det["n_trials"].max()) <= svtav1_hip.sgrproj_walk_max_trials()
    assert D.inputs_untouched()
    # the search's device-side result feeds the frame filter without a round trip: run 0 of the fixture
    d_type = _dev(torch, F["utype"][0])
    _ready(torch)
    hip_ctx.av1_lr_filter_frame_dev(D.pic, D.out.ptr, D.out.stride, 0, 3, d_type.data_ptr(), None, d_sgr.data_ptr(), bit_depth=F["bd"])
    hip_ctx.synchronize()
    got, guard_ok = D.out.planes()
    assert guard_ok and all(np.array_equal(got[p], F["out"][0][p]) for p in range(3)), c
    assert hip_ctx.inter_pred_refused() == 0


def test_chroma_only_search_with_null_luma(hip_ctx):
    torch = pytest.importorskip("torch")
    F = fixture_case(4)
    D = _case(torch, F)
    b = F["base"]
    cb = svtav1_hip.make_lr_picture(F["w"], F["h"], [None, D.cdef.ptr[1], None], D.cdef.stride, [None, D.dbk.ptr[1], None], D.dbk.stride,
                                    [None, D.src.ptr[1], None], D.src.stride)
    d_sgr, d_sse, d_det = _search(torch, hip_ctx, D, 1, 2, pic=cb)
    hip_ctx.synchronize()
    sgr, sse = d_sgr.cpu().numpy(), d_sse.cpu().numpy()
    det = d_det.cpu().numpy().reshape(D.n, 16 * 80)
    assert np.array_equal(sgr[b[1]:b[2]], F["sgrproj"][b[1]:b[2]]) and np.array_equal(sse[b[1]:b[2]], F["sse"][b[1]:b[2]])
    assert (sgr[:b[1]] == -1).all() and (sgr[b[2]:] == -1).all() and (sse[:b[1]] == -1).all() and (sse[b[2]:] == -1).all()
    assert (det[:b[1]] == 0xEE).all() and (det[b[2]:] == 0xEE).all()
    assert np.array_equal(det[b[1]:b[2]].copy().view(svtav1_hip.SGRPROJ_DETAIL_DTYPE).reshape(-1, 16)["err"], F["detail"]["err"][b[1]:b[2]])
    # without the records
    d_sgr2, _, _ = _search(torch, hip_ctx, D, 1, 2, pic=cb, detail=False)
    hip_ctx.synchronize()
    assert np.array_equal(d_sgr2.cpu().numpy(), sgr)
    assert D.inputs_untouched()


@pytest.mark.parametrize("c", range(N_CASES))
def test_trial_sse_matches_fixture(hip_ctx, c):
    """the SSE of the search's filter; with a skip mask; of the filters of the other runs against the restatement"""
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = _case(torch, F)
    d_sgr = _dev(torch, F["sgrproj"])
    d_sse = torch.full((D.n,), -1, dtype=torch.int64, device="cuda:0")
    _ready(torch)
    hip_ctx.av1_sgrproj_trial_sse_dev(D.pic, 0, 3, d_sgr.data_ptr(), d_sse.data_ptr(), None, bit_depth=F["bd"])
    hip_ctx.synchronize()
    assert np.array_equal(d_sse.cpu().numpy(), F["sse"])
    skip = np.zeros(D.n, np.uint8)
    skip[F["base"][1]] = 1
    d_skip = _dev(torch, skip)
    d_sse.fill_(-1)
    _ready(torch)
    hip_ctx.av1_sgrproj_trial_sse_dev(D.pic, 1, 3, d_sgr.data_ptr(), d_sse.data_ptr(), d_skip.data_ptr(), bit_depth=F["bd"])
    hip_ctx.synchronize()
    want = F["sse"].copy()
    want[:F["base"][1]], want[F["base"][1]] = -1, 0
    assert np.array_equal(d_sse.cpu().numpy(), want)
    # the extreme parameters of run 2: the frame run's output minus the source, squared, is the unit's SSE
    d_sgr2 = _dev(torch, F["usgr"][2])
    _ready(torch)
    hip_ctx.av1_sgrproj_trial_sse_dev(D.pic, 1, 3, d_sgr2.data_ptr(), d_sse.data_ptr(), None, bit_depth=F["bd"])
    hip_ctx.synchronize()
    got = d_sse.cpu().numpy()
    for p in (1, 2):
        for i, lim in enumerate(F["limits"][p]):
            h0, h1, v0, v1 = (int(v) for v in lim)
            d = F["out"][2][p][v0:v1, h0:h1].astype(np.int64) - F["src"][p][v0:v1, h0:h1].astype(np.int64)
            assert int(got[F["base"][p] + i]) == int((d * d).sum()), (c, p, i)
    assert D.inputs_untouched()


@pytest.mark.parametrize("c", range(N_CASES))
def test_frame_filter_matches_every_run(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    for r in range(len(F["ftype"])):
        D = _case(torch, F)
        ps = 0 if F["ftype"][r][0] else 1
        d_type, d_taps, d_sgr = _dev(torch, F["utype"][r]), _dev(torch, F["utaps"][r]), _dev(torch, F["usgr"][r])
        _ready(torch)
        hip_ctx.av1_lr_filter_frame_dev(D.pic, D.out.ptr, D.out.stride, ps, 3, d_type.data_ptr(), d_taps.data_ptr(), d_sgr.data_ptr(), bit_depth=F["bd"])
        hip_ctx.synchronize()
        got, guard_ok = D.out.planes()
        for p in range(3):
            want = F["out"][r][p] if F["ftype"][r][p] else np.full_like(F["cdef"][p], 7)
            assert np.array_equal(got[p], want), (c, r, p)
        assert guard_ok and D.inputs_untouched(), (c, r)
        assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("bad", ((16, 0, 0, 0), (-1, 0, 0, 0), (3, 32, 0, 0), (3, 0, -33, 0)))
def test_bad_parameters_are_refused_on_the_device(hip_ctx, bad):
    """a set above 15 or an xqd outside its range: counted once, nothing of the unit written, the other units as the fixture has them"""
    torch = pytest.importorskip("torch")
    F = fixture_case(1)
    D = _case(torch, F)
    sgr = F["usgr"][0].copy()
    sgr[1] = bad
    assert hip_ctx.inter_pred_refused() == 0
    d_type, d_sgr = _dev(torch, F["utype"][0]), _dev(torch, sgr)
    _ready(torch)
    hip_ctx.av1_lr_filter_frame_dev(D.pic, D.out.ptr, D.out.stride, 0, 3, d_type.data_ptr(), None, d_sgr.data_ptr(), bit_depth=F["bd"])
    hip_ctx.synchronize()
    with pytest.raises(svtav1_hip.SvtHipError, match=r": 1 PU\(s\) or unit\(s\) refused"):
        hip_ctx.inter_pred_refused()
    assert hip_ctx.inter_pred_refused() == 0
    got, guard_ok = D.out.planes()
    h0, h1, v0, v1 = (int(v) for v in F["limits"][0][1])
    want = F["out"][0][0].copy()
    want[v0:v1, h0:h1] = 7
    assert guard_ok and np.array_equal(got[0], want) and np.array_equal(got[1], F["out"][0][1]) and np.array_equal(got[2], F["out"][0][2])
    # the SSE trial marks such a unit with -1
    d_sse = torch.full((D.n,), -5, dtype=torch.int64, device="cuda:0")
    _ready(torch)
    hip_ctx.av1_sgrproj_trial_sse_dev(D.pic, 0, 1, d_sgr.data_ptr(), d_sse.data_ptr(), None, bit_depth=F["bd"])
    hip_ctx.synchronize()
    sse = d_sse.cpu().numpy()
    assert sse[1] == -1 and sse[0] == F["sse"][0] and (sse[2:] == -5).all()


def test_missing_taps_or_parameters_are_refused_on_the_device(hip_ctx):
    """the mixed run without d_taps: its Wiener units are refused; without d_sgrproj: its self-guided units are"""
    torch = pytest.importorskip("torch")
    F = fixture_case(1)
    types = F["utype"][1]
    for missing, kind in (("taps", svtav1_hip.RESTORE_WIENER), ("sgr", svtav1_hip.RESTORE_SGRPROJ)):
        D = _case(torch, F)
        d_type, d_taps, d_sgr = _dev(torch, types), _dev(torch, F["utaps"][1]), _dev(torch, F["usgr"][1])
        _ready(torch)
        hip_ctx.av1_lr_filter_frame_dev(D.pic, D.out.ptr, D.out.stride, 0, 3, d_type.data_ptr(), None if missing == "taps" else d_taps.data_ptr(),
                                        None if missing == "sgr" else d_sgr.data_ptr(), bit_depth=F["bd"])
        hip_ctx.synchronize()
        n_bad = int((types == kind).sum())
        assert n_bad > 0
        with pytest.raises(svtav1_hip.SvtHipError, match=rf": {n_bad} PU\(s\) or unit\(s\) refused"):
            hip_ctx.inter_pred_refused()
        got, guard_ok = D.out.planes()
        assert guard_ok
        for p in range(3):
            want = F["out"][1][p].copy()
            for i, lim in enumerate(F["limits"][p]):
                if types[F["base"][p] + i] == kind:
                    h0, h1, v0, v1 = (int(v) for v in lim)
                    want[v0:v1, h0:h1] = 7
            assert np.array_equal(got[p], want), (missing, p)


def test_refusals(hip_ctx):
    """refused on the host, before any launch: nothing is written"""
    torch = pytest.importorskip("torch")
    F = fixture_case(0)
    D = _case(torch, F)
    n = D.n
    d64 = torch.full((n * 16 * 10 + 8,), -1, dtype=torch.int64, device="cuda:0")
    d32 = torch.full((64 * 80,), -1, dtype=torch.int32, device="cuda:0")
    d8 = _dev(torch, F["utype"][0])
    w, h = F["w"], F["h"]
    mk = lambda **k: svtav1_hip.make_lr_picture(k.get("w", w), k.get("h", h), k.get("cdef", D.cdef.ptr), D.cdef.stride, D.dbk.ptr,  # noqa: E731
                                                k.get("dstride", D.dbk.stride), D.src.ptr, D.src.stride, k.get("unit"))
    odd, unit96, no_cb, narrow = mk(w=w - 4), mk(unit=(128, 96, 64)), mk(cdef=[D.cdef.ptr[0], None, D.cdef.ptr[2]]), mk(dstride=[8, 8, 8])
    search = lambda pic, ps=0, pe=3, bd=F["bd"], work=D.work.data_ptr(), sgr=d32.data_ptr(), det=None: hip_ctx.av1_search_sgrproj_dev(  # noqa: E731
        pic, ps, pe, work, sgr, d64.data_ptr(), det, bit_depth=bd)
    trial = lambda pic, ps=0, pe=3, bd=F["bd"], sgr=d32.data_ptr(), sse=d64.data_ptr(): hip_ctx.av1_sgrproj_trial_sse_dev(  # noqa: E731
        pic, ps, pe, sgr, sse, None, bit_depth=bd)
    frame = lambda pic, ps=0, pe=3, out=D.out.ptr, types=d8.data_ptr(), bd=F["bd"], sgr=d32.data_ptr(): hip_ctx.av1_lr_filter_frame_dev(  # noqa: E731
        pic, out, D.out.stride, ps, pe, types, None, sgr, bit_depth=bd)
    plane = lambda pic, p=0, ep=0, bd=F["bd"], f0=d32.data_ptr(), f1=d32.data_ptr(), stride=64: hip_ctx.av1_selfguided_restoration_dev(  # noqa: E731
        pic, p, ep, f0, f1, stride, bit_depth=bd)
    calls = []
    for f in (search, trial, frame):
        calls += [lambda f=f: f(odd), lambda f=f: f(unit96), lambda f=f: f(no_cb), lambda f=f: f(narrow), lambda f=f: f(None),
                  lambda f=f: f(D.pic, 1, 1), lambda f=f: f(D.pic, 2, 1), lambda f=f: f(D.pic, 0, 4), lambda f=f: f(D.pic, bd=12),
                  lambda f=f: f(D.pic, sgr=d32.data_ptr() + 2)]
    calls += [lambda: plane(odd), lambda: plane(unit96), lambda: plane(no_cb, 1), lambda: plane(narrow), lambda: plane(None), lambda: plane(D.pic, 3),
              lambda: plane(D.pic, 0, 16), lambda: plane(D.pic, bd=12), lambda: plane(D.pic, stride=63), lambda: plane(D.pic, 1, 0, stride=31),
              lambda: plane(D.pic, f0=None), lambda: plane(D.pic, f1=None), lambda: plane(D.pic, 0, 12, f1=None), lambda: plane(D.pic, 0, 15, f0=None),
              lambda: plane(D.pic, f0=d32.data_ptr() + 2),
              lambda: search(D.pic, work=None), lambda: search(D.pic, sgr=None), lambda: search(D.pic, work=D.work.data_ptr() + 4),
              lambda: search(D.pic, det=d64.data_ptr() + 4), lambda: trial(D.pic, sgr=None), lambda: trial(D.pic, sse=None),
              lambda: trial(D.pic, sse=d64.data_ptr() + 4), lambda: frame(D.pic, types=None),
              lambda: hip_ctx.av1_lr_filter_frame_dev(D.pic, D.out.ptr, D.out.stride, 0, 3, d8.data_ptr(), d32.data_ptr() + 1, d32.data_ptr(),
                                                      bit_depth=F["bd"]),
              lambda: frame(D.pic, out=[D.out.ptr[0], None, D.out.ptr[2]]),
              lambda: hip_ctx.sgrproj_solve_dev(None, d32.data_ptr(), d32.data_ptr(), 1, d32.data_ptr(), d32.data_ptr()),
              lambda: hip_ctx.sgrproj_solve_dev(d64.data_ptr(), d32.data_ptr(), d32.data_ptr(), 1, None, d32.data_ptr()),
              lambda: hip_ctx.sgrproj_solve_dev(d64.data_ptr() + 4, d32.data_ptr(), d32.data_ptr(), 1, d32.data_ptr(), d32.data_ptr()),
              lambda: hip_ctx.sgrproj_solve_dev(d64.data_ptr(), d32.data_ptr() + 2, d32.data_ptr(), 1, d32.data_ptr(), d32.data_ptr()),
              lambda: hip_ctx.sgrproj_walk_table_dev(None, d32.data_ptr(), d32.data_ptr(), 1, d32.data_ptr(), d64.data_ptr(), d32.data_ptr()),
              lambda: hip_ctx.sgrproj_walk_table_dev(d64.data_ptr(), d32.data_ptr(), d32.data_ptr(), 1, d32.data_ptr(), None, d32.data_ptr()),
              lambda: hip_ctx.sgrproj_walk_table_dev(d64.data_ptr(), d32.data_ptr(), d32.data_ptr(), 1, d32.data_ptr(), d64.data_ptr() + 4, d32.data_ptr())]
    for i, call in enumerate(calls):
        with pytest.raises(svtav1_hip.SvtHipError):
            call()
    hip_ctx.synchronize()
    got, guard_ok = D.out.planes()
    assert guard_ok and all((g == 7).all() for g in got) and D.inputs_untouched()
    assert bool((d64 == -1).all()) and bool((d32 == -1).all())
    # the planes of a call are the only ones checked (a radius-0 pointer may be null), and the two host numbers
    plane(no_cb, 0, 12, f0=None)
    hip_ctx.synchronize()
    assert int(d32.cpu()[0]) != -1
    assert svtav1_hip.sgrproj_walk_max_trials() == 131
