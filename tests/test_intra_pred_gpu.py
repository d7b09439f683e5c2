"""GPU: svthip_av1_[highbd_]intra_pred_batch_dev (AV1 intra prediction of transform blocks) bit-exact against the reference's fixture
(tests/golden/intra_pred.npz) and against the numpy restatement on random batches of every TxSize at both depths; edges read in place from
a plane in wavefront order; the optional SAD; every refusal on the host and on the device; the caller-stream contract."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import intra_pred_util as iu  # noqa: E402
import paeth_vectors as pv  # noqa: E402
import svtav1_hip  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "intra_pred.npz")


def _bad(got, want, per):
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else (len(bad), bad[:4] // per, got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("bd", [8, 10])
def test_fixture_bit_exact(hip_ctx, bd):
    pytest.importorskip("torch")
    g = np.load(GOLDEN)
    desc_all = g["desc"].view(iu.DESC)
    sizes = set()
    for (ts, cbd, d0, dn, e0, en, o0, on) in g["case"]:
        if cbd != bd:
            continue
        txw, txh = iu.TX_SIZES_WH[ts]
        edge, desc, want = g[f"edge_{bd}"][e0:e0 + en], desc_all[d0:d0 + dn], g[f"out_{bd}"][o0:o0 + on]
        dst = np.full(len(want), iu.FILL[bd], edge.dtype)
        got, _ = iu.run_device(hip_ctx, edge, dst, desc, int(ts), bd)
        assert _bad(got, want, txw * txh) is None, (ts, bd, _bad(got, want, txw * txh))
        sizes.add(int(ts))
    assert len(sizes) == 19
    assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("tx_size", range(19))
def test_random_batches_match_restatement(hip_ctx, tx_size, bd):
    pytest.importorskip("torch")
    txw, txh = iu.TX_SIZES_WH[tx_size]
    n = 203 if txw * txh <= 256 else 37 if txw * txh <= 1024 else 11     # no multiple of the 4 .. 64 blocks of a workgroup
    edge, desc, _ = iu.random_case(np.random.default_rng(100 * tx_size + bd), n, tx_size, bd)
    desc["mode"][:3] = iu.PAETH       # the reference has no PAETH: every batch carries it, and all three winners must occur
    assert len(set(desc["mode"])) > 6 and len(set(desc["angle_delta"])) > 3
    want = np.full(n * txw * txh, iu.FILL[bd], edge.dtype)
    stats = iu.new_stats()
    assert iu.predict(edge, want, desc, tx_size, bd, stats=stats)[0] == 0
    assert stats["paeth"] == {"left", "top", "topleft"}
    got, _ = iu.run_device(hip_ctx, edge, np.full_like(want, iu.FILL[bd]), desc, tx_size, bd)
    assert _bad(got, want, txw * txh) is None, (tx_size, bd, _bad(got, want, txw * txh))
    assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_paeth_vectors(hip_ctx, bd):
    """mode 12 against vectors worked from the specification's rule (tests/paeth_vectors.py), not against the restatement"""
    pytest.importorskip("torch")
    for ts in pv.SIZES:
        txw, txh = iu.TX_SIZES_WH[ts]
        edge, desc, want, winners = pv.vectors(ts, bd)
        assert winners == {"left", "top", "topleft"}
        got, _ = iu.run_device(hip_ctx, edge, np.full_like(want, iu.FILL[bd]), desc, ts, bd)
        assert _bad(got, want, txw * txh) is None, (ts, bd, _bad(got, want, txw * txh))
    assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_unaligned_destinations(hip_ctx, bd):
    """odd destination offsets and strides: the per-sample store path"""
    pytest.importorskip("torch")
    for tx_size in (0, 14, 2):
        txw, txh = iu.TX_SIZES_WH[tx_size]
        n = 21
        edge, desc, _ = iu.random_case(np.random.default_rng(7 + tx_size + bd), n, tx_size, bd)
        desc["dst_stride"] = txw + 3
        desc["dst_offset"] = np.arange(n) * (txw + 3) * txh + np.arange(n) % 4
        want = np.full(n * (txw + 3) * txh + 8, iu.FILL[bd], edge.dtype)
        iu.predict(edge, want, desc, tx_size, bd)
        got, _ = iu.run_device(hip_ctx, edge, np.full_like(want, iu.FILL[bd]), desc, tx_size, bd)
        assert np.array_equal(got, want), (tx_size, bd)


def _raster_descs(W, H, S, diag, rng):
    """8x8 blocks of anti-diagonal `diag` of a W x H plane with stride S: edges straight from the plane"""
    out = []
    for by in range(H // 8):
        bx = diag - by
        if not 0 <= bx < W // 8:
            continue
        x, y = 8 * bx, 8 * by
        d = np.zeros(1, iu.DESC)[0]
        d["above_offset"] = (y - 1) * S + x if y else 0
        d["left_offset"] = y * S + x - 1 if x else 0
        d["left_stride"] = S
        d["dst_offset"], d["dst_stride"] = y * S + x, S
        d["n_top_px"] = 8 if y else 0
        d["n_left_px"] = 8 if x else 0
        # the blocks above-right and below-left lie on this same anti-diagonal, so they are written by this call: not available
        d["mode"], d["angle_delta"] = rng.integers(0, 13), rng.integers(-3, 4)
        out.append(d)
    return np.array(out, iu.DESC)


@pytest.mark.parametrize("bd", [8, 10])
def test_in_place_wavefront_over_a_plane(hip_ctx, bd):
    torch = pytest.importorskip("torch")
    W, H, S = 64, 48, 72
    dt = np.uint8 if bd == 8 else np.uint16
    plane = np.full(S * H, iu.FILL[bd], dt)
    want = plane.copy()
    d_plane = torch.from_numpy(plane if bd == 8 else plane.view(np.int16)).to("cuda:0")
    rng = np.random.default_rng(31 + bd)
    for diag in range(W // 8 + H // 8 - 1):
        desc = _raster_descs(W, H, S, diag, rng)
        iu.predict(want, want, desc, 1, bd)
        d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        if bd == 8:
            hip_ctx.av1_intra_pred_batch_dev(d_plane.data_ptr(), d_plane.data_ptr(), d_desc.data_ptr(), len(desc), 1)
        else:
            hip_ctx.av1_highbd_intra_pred_batch_dev(d_plane.data_ptr(), d_plane.data_ptr(), d_desc.data_ptr(), len(desc), 1, 10)
    hip_ctx.synchronize()
    got = d_plane.cpu().numpy().view(dt)
    assert np.array_equal(got, want)
    assert not np.array_equal(got.reshape(H, S)[:, :W], np.full((H, W), iu.FILL[bd], dt))
    assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("tx_size", [0, 2, 18, 4])
def test_sad_and_prediction_unchanged_by_it(hip_ctx, tx_size):
    pytest.importorskip("torch")
    txw, txh = iu.TX_SIZES_WH[tx_size]
    n = 67 if txw * txh <= 256 else 9
    edge, desc, src = iu.random_case(np.random.default_rng(900 + tx_size), n, tx_size, 8)
    want = np.full(n * txw * txh, iu.FILL[8], np.uint8)
    _, want_sad = iu.predict(edge, want, desc, tx_size, 8, src=src)
    plain, none = iu.run_device(hip_ctx, edge, np.full_like(want, iu.FILL[8]), desc, tx_size, 8)
    got, sad = iu.run_device(hip_ctx, edge, np.full_like(want, iu.FILL[8]), desc, tx_size, 8, src=src, want_sad=True)
    assert none is None and np.array_equal(plain, want) and np.array_equal(got, want)
    assert np.array_equal(sad, want_sad)


def test_host_refusals(hip_ctx):
    torch = pytest.importorskip("torch")
    E = svtav1_hip.SvtHipError
    edge, desc, src = iu.random_case(np.random.default_rng(1), 8, 1, 8)
    d_e = torch.from_numpy(edge).to("cuda:0")
    d_o = torch.zeros(8 * 64, dtype=torch.uint8, device="cuda:0")
    d_d = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_s = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    e, o, d = d_e.data_ptr(), d_o.data_ptr(), d_d.data_ptr()
    for ts in (19, 255):
        with pytest.raises(E, match="tx_size"):
            hip_ctx.av1_intra_pred_batch_dev(e, o, d, 8, ts)
        with pytest.raises(E, match="tx_size"):
            hip_ctx.av1_highbd_intra_pred_batch_dev(e, o, d, 8, ts, 10)
    for args in ((None, o, d), (e, None, d), (e, o, None)):
        with pytest.raises(E, match="null"):
            hip_ctx.av1_intra_pred_batch_dev(*args, 8, 1)
        with pytest.raises(E, match="null"):
            hip_ctx.av1_highbd_intra_pred_batch_dev(*args, 8, 1, 10)
    with pytest.raises(E, match="16-byte"):
        hip_ctx.av1_intra_pred_batch_dev(e, o, buf.data_ptr() + 4, 8, 1)
    for bad_bd in (8, 12):
        with pytest.raises(E, match="bit_depth"):
            hip_ctx.av1_highbd_intra_pred_batch_dev(e, o, d, 8, 1, bad_bd)
    with pytest.raises(E, match="d_src"):
        hip_ctx.av1_intra_pred_batch_dev(e, o, d, 8, 1, None, d_s.data_ptr())
    hip_ctx.av1_intra_pred_batch_dev(None, None, None, 0, 1)           # n_blocks == 0: OK
    hip_ctx.av1_highbd_intra_pred_batch_dev(None, None, None, 0, 1, 10)
    assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_device_refusals_leave_the_destination(hip_ctx, bd):
    pytest.importorskip("torch")
    E = svtav1_hip.SvtHipError
    for tx_size in (0, 8, 4):
        txw, txh = iu.TX_SIZES_WH[tx_size]
        n = 23
        edge, desc, _ = iu.random_case(np.random.default_rng(55 + tx_size), n, tx_size, bd)
        desc["n_top_px"][:12], desc["n_left_px"][:12], desc["n_topright_px"][:12], desc["n_bottomleft_px"][:12] = txw, txh, 0, 0
        desc[0]["mode"] = 13
        desc[2]["angle_delta"] = 4
        desc[3]["angle_delta"] = -4
        desc[5]["n_top_px"] = txw + 1
        desc[6]["n_left_px"] = txh + 1
        desc[7]["n_top_px"], desc[7]["n_topright_px"] = txw - 1, 1
        desc[8]["n_left_px"], desc[8]["n_bottomleft_px"] = txh - 1, 1
        desc[9]["n_topright_px"] = txw + 1
        desc[n - 1]["mode"] = 200
        n_bad = 9
        want = np.full(n * txw * txh, iu.FILL[bd], edge.dtype)
        assert iu.predict(edge, want, desc, tx_size, bd)[0] == n_bad
        got, _ = iu.run_device(hip_ctx, edge, np.full_like(want, iu.FILL[bd]), desc, tx_size, bd)
        assert np.array_equal(got, want)
        for i in (0, 2, 3, 5, 6, 7, 8, 9, n - 1):
            assert (got[i * txw * txh:(i + 1) * txw * txh] == iu.FILL[bd]).all()
        with pytest.raises(E, match=f"{n_bad} PU"):
            hip_ctx.inter_pred_refused()
        assert hip_ctx.inter_pred_refused() == 0


def test_caller_stream_without_synchronisation(hip_ctx):
    torch = pytest.importorskip("torch")
    for bd, tx_size in ((8, 0), (10, 1), (8, 4), (10, 18)):
        txw, txh = iu.TX_SIZES_WH[tx_size]
        n = 37
        edge, desc, _ = iu.random_case(np.random.default_rng(70 + tx_size), n, tx_size, bd)
        want = np.full(n * txw * txh, iu.FILL[bd], edge.dtype)
        iu.predict(edge, want, desc, tx_size, bd)
        s = torch.cuda.Stream()
        as_t = (lambda a: torch.from_numpy(a.copy())) if bd == 8 else (lambda a: torch.from_numpy(a.view(np.int16).copy()))
        d_e, d_o = as_t(edge).to("cuda:0"), as_t(np.full_like(want, iu.FILL[bd])).to("cuda:0")
        d_d = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        s.wait_stream(torch.cuda.current_stream())   # stream order, not a host wait
        with torch.cuda.stream(s):
            if bd == 8:
                hip_ctx.av1_intra_pred_batch_dev(d_e.data_ptr(), d_o.data_ptr(), d_d.data_ptr(), n, tx_size, stream=s.cuda_stream)
            else:
                hip_ctx.av1_highbd_intra_pred_batch_dev(d_e.data_ptr(), d_o.data_ptr(), d_d.data_ptr(), n, tx_size, 10, stream=s.cuda_stream)
            host = d_o.to("cpu")   # enqueued on s behind the prediction
        got = host.numpy() if bd == 8 else host.numpy().view(np.uint16)
        assert np.array_equal(got, want), (bd, tx_size)
    assert hip_ctx.inter_pred_refused() == 0
