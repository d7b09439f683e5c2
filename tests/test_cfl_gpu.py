"""GPU: svthip_av1_[highbd_]cfl_pred_batch_dev, svthip_av1_cfl_alpha_candidates_batch_dev and svthip_cfl_alpha_decision_batch_dev bit-exact
against the reference's fixture (tests/golden/cfl.npz) and against the numpy restatement (tests/cfl_util.py) on random batches of every
luma shape at both depths; in-place and separate destinations, odd offsets and strides; the candidate pool against predict mode; the
decision against the reference's recorded walk and on random tables, with everything outside the returned masks overwritten; the whole
search composed with the fused chain and the coefficient rate on the device; every refusal; the caller-stream contract."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import cfl_util as cu  # noqa: E402
import svtav1_hip  # noqa: E402
from test_cfl_vs_ref import fixture_cases, fixture_decisions  # noqa: E402

pytestmark = pytest.mark.gpu


def _n_jobs(lw, lh):
    return 203 if lw * lh <= 256 else 37     # no multiple of the 4 .. 64 blocks of a workgroup


@pytest.mark.parametrize("bd", [8, 10])
def test_fixture_bit_exact(hip_ctx, bd):
    pytest.importorskip("torch")
    shapes = set()
    for (lw, lh, cbd, luma, cb, cr, desc, want_cb, want_cr, _) in fixture_cases():
        if cbd != bd:
            continue
        got_cb, got_cr = cu.run_device(hip_ctx, luma, cb, cr, desc, lw, lh, bd)
        assert np.array_equal(got_cb, want_cb) and np.array_equal(got_cr, want_cr), (lw, lh, bd)
        shapes.add((lw, lh))
    assert len(shapes) == 9
    assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("shape", cu.LUMA_SIZES_WH)
def test_random_batches_match_restatement(hip_ctx, shape, bd):
    """in place, then into separate planes that keep their filling wherever no block lies"""
    pytest.importorskip("torch")
    lw, lh = shape
    n = _n_jobs(lw, lh)
    luma, cb, cr, desc = cu.random_case(np.random.default_rng(100 * lw + lh + bd), n, lw, lh, bd)
    want_cb, want_cr = cb.copy(), cr.copy()
    assert cu.predict(luma, cb, cr, want_cb, want_cr, desc, lw, lh, bd) == 0
    got_cb, got_cr = cu.run_device(hip_ctx, luma, cb, cr, desc, lw, lh, bd)
    assert np.array_equal(got_cb, want_cb) and np.array_equal(got_cr, want_cr), (shape, bd)
    fill_cb, fill_cr = np.full_like(cb, cu.FILL[bd]), np.full_like(cr, cu.FILL[bd] + 1)
    want_cb, want_cr = fill_cb.copy(), fill_cr.copy()
    cu.predict(luma, cb, cr, want_cb, want_cr, desc, lw, lh, bd)
    got_cb, got_cr = cu.run_device(hip_ctx, luma, cb, cr, desc, lw, lh, bd, in_place=False, cb_dst=fill_cb, cr_dst=fill_cr)
    assert np.array_equal(got_cb, want_cb) and np.array_equal(got_cr, want_cr), (shape, bd)
    assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_unaligned_positions(hip_ctx, bd):
    """odd chroma offsets and strides (the per-sample load and store paths) and a luma plane that starts at an odd sample"""
    pytest.importorskip("torch")
    for (lw, lh) in ((8, 8), (32, 8), (16, 32), (32, 32)):
        n = 21
        luma, cb, cr, desc = cu.random_case(np.random.default_rng(7 + lw + lh + bd), n, lw, lh, bd, chroma_pad=3, odd_offsets=True)
        luma = np.concatenate([luma[:3], luma])
        desc["luma_offset"] += 3
        want_cb, want_cr = cb.copy(), cr.copy()
        cu.predict(luma, cb, cr, want_cb, want_cr, desc, lw, lh, bd)
        got_cb, got_cr = cu.run_device(hip_ctx, luma, cb, cr, desc, lw, lh, bd)
        assert np.array_equal(got_cb, want_cb) and np.array_equal(got_cr, want_cr), (lw, lh, bd)


@pytest.mark.parametrize("shape", cu.LUMA_SIZES_WH)
def test_candidates_equal_predict_mode(hip_ctx, shape):
    """every tile of the pool is what predict mode writes with that alpha (through the restatement, which the tests above hold the predict
    entry to, and for three alphas through the predict entry itself); jobs beyond n_blocks stay untouched"""
    torch = pytest.importorskip("torch")
    lw, lh = shape
    cw, ch = lw // 2, lh // 2
    n = 19 if lw * lh <= 256 else 7
    luma, cb, cr, desc = cu.random_case(np.random.default_rng(300 + lw * 64 + lh), n + 2, lw, lh, 8, chroma_pad=5)
    want = cu.candidates(luma, cb, cr, desc[:n], lw, lh)
    d_pool = torch.full(((n + 2) * 66 * cw * ch,), 0xa5, dtype=torch.uint8, device="cuda:0")
    d_l, d_cb, d_cr, d_desc = cu.to_dev(luma), cu.to_dev(cb), cu.to_dev(cr), cu.to_dev(desc)
    hip_ctx.av1_cfl_alpha_candidates_batch_dev(d_l.data_ptr(), d_cb.data_ptr(), d_cr.data_ptr(), d_desc.data_ptr(), n, lw, lh, d_pool.data_ptr())
    hip_ctx.synchronize()
    got = d_pool.cpu().numpy().reshape(n + 2, 2, 33, ch * cw)
    assert np.array_equal(got[:n], want), shape
    assert (got[n:] == 0xa5).all()
    assert np.array_equal(d_cb.cpu().numpy(), cb) and np.array_equal(d_cr.cpu().numpy(), cr)
    at = np.arange(ch)[:, None] * int(desc[0]["chroma_stride"]) + np.arange(cw)[None, :]
    for (a_u, a_v) in ((-16, 16), (5, -1), (0, 9)):
        d = desc[:n].copy()
        d["alpha_idx"], d["alpha_signs"] = cu.alpha_to_fields(a_u, a_v)
        pcb, pcr = cu.run_device(hip_ctx, luma, cb, cr, d, lw, lh, 8)
        for i in range(n):
            assert np.array_equal(got[i, 0, a_u + 16].reshape(ch, cw), pcb[int(d[i]["cb_offset"]) + at])
            assert np.array_equal(got[i, 1, a_v + 16].reshape(ch, cw), pcr[int(d[i]["cr_offset"]) + at])


def _poison_outside(dist, bits, decisions):
    d2, b2 = dist.copy(), bits.copy()
    k = np.arange(33, dtype=np.uint64)
    for i, o in enumerate(decisions):
        for p in range(2):
            out = ((np.uint64(o["evaluated_mask"][p]) >> k) & np.uint64(1)) == 0
            d2[i, p, out] = 0xffffffffffffffff
            b2[i, p, out] = 0xffffffff
    return d2, b2


def test_decision_matches_the_reference_walk(hip_ctx):
    pytest.importorskip("torch")
    ab, group, dist, bits, jobs, want_out, want_mask, shift = fixture_decisions()
    for g in range(len(ab)):
        sel = np.flatnonzero(group == g)
        got = cu.run_device_decision(hip_ctx, dist[sel], bits[sel], shift, ab[g], jobs[sel])
        assert np.array_equal(np.stack([got["intra_chroma_mode"], got["cfl_alpha_idx"], got["cfl_alpha_signs"]], 1), want_out[sel]), g
        assert np.array_equal(got["evaluated_mask"], want_mask[sel]), g
        assert not got["reserved"].any()
        d2, b2 = _poison_outside(dist[sel], bits[sel], got)
        assert np.array_equal(cu.run_device_decision(hip_ctx, d2, b2, shift, ab[g], jobs[sel]), got), g


@pytest.mark.parametrize("dist_shift", [0, 2, 63])
def test_decision_on_random_tables(hip_ctx, dist_shift):
    pytest.importorskip("torch")
    rng = np.random.default_rng(40 + dist_shift)
    ab = cu.random_alpha_bits(rng)
    dist, bits, jobs = cu.random_decision_tables(rng, 203)      # more than three workgroups of 64 lanes, the last one partial
    stats = cu.new_decision_stats()
    want = cu.decide_batch(dist, bits, dist_shift, ab, jobs, stats)
    assert dist_shift == 63 or (len(stats["winners"]) >= 6 and stats["dc_wins"] and stats["exit_c"] and stats["full_runs"])
    got = cu.run_device_decision(hip_ctx, dist, bits, dist_shift, ab, jobs)
    assert np.array_equal(got, want)
    d2, b2 = _poison_outside(dist, bits, got)
    assert np.array_equal(cu.run_device_decision(hip_ctx, d2, b2, dist_shift, ab, jobs), got)


def test_whole_search_on_the_device(hip_ctx, oracle):
    """candidates -> fused chain on the pool (one descriptor per tile, DCT_DCT) -> coefficient rate -> decision, all on the device, against
    the same composition made of the restated candidates, the oracle's chain, the restated rate and the restated walk"""
    torch = pytest.importorskip("torch")
    import rate_util
    import tq_util

    rng = np.random.default_rng(77)
    n, lw, lh, cw, ch, ts = 6, 16, 16, 8, 8, 1
    luma, cb, cr, desc = cu.random_case(rng, n, lw, lh, 8, kinds=(0, 1))
    # chroma sources that follow the luma AC with a different alpha per block and plane, so that CfL has something to find
    src = np.zeros((n, 2, ch * cw), np.uint8)
    at = np.arange(ch)[:, None] * cw + np.arange(cw)[None, :]
    for i, d in enumerate(desc):
        ac = cu.block_ac(luma, d, lw, lh, 8)
        for p, (plane, off) in enumerate(((cb, d["cb_offset"]), (cr, d["cr_offset"]))):
            a = ((0, 0), (-7, 3), (12, -16), (1, 0), (0, 0), (3, -7))[i][p]
            src[i, p] = np.clip(plane[int(off) + at] + ((a * ac) >> 6) + rng.integers(-2, 3, (ch, cw)), 0, 255).reshape(-1)
    tabs = tq_util.RealTables()
    z = np.load(os.path.join(ROOT, "tests", "golden", "coeff_rate.npz"))
    T = z["tables"].view(svtav1_hip.COEFF_RATE_TABLES_DTYPE).reshape(-1)
    n_tu, npx = n * 66, cw * ch
    t = np.arange(n_tu)
    tu = np.zeros(n_tu, svtav1_hip.TU_DESC_DTYPE)
    tu["src_offset"] = (t // 33) * npx
    tu["pred_offset"] = tu["recon_offset"] = tu["coeff_offset"] = t * npx
    tu["src_stride"] = tu["pred_stride"] = tu["recon_stride"] = cw
    tu["iscan_offset"] = tabs.scan_offset(ts, 0)
    tu["qparam_index"] = (t // 66) % 2
    qparams = np.ascontiguousarray(tabs.rows(8, "inter")[[60, 140], 1, :])
    rd = np.zeros(n_tu, svtav1_hip.COEFF_RATE_DESC_DTYPE)
    rd["coeff_offset"], rd["iscan_offset"], rd["plane_type"], rd["intra_mode"] = t * npx, tabs.scan_offset(ts, 0), 1, 0
    ab = cu.random_alpha_bits(rng)
    jobs = np.zeros(n, cu.JOB)
    jobs["lambda"], jobs["cfl_mode_bits"], jobs["dc_mode_bits"] = rng.integers(200, 3000, n), 900, 400
    shift = rate_util.tx_scale_shift(ts)

    # the composition on the CPU
    pool = cu.candidates(luma, cb, cr, desc, lw, lh)
    b = {"src": src.reshape(-1), "pred": pool.reshape(-1), "desc": tu, "qparams": qparams, "scan": tabs.scan_pool, "iscan": tabs.iscan_pool,
         "w": cw, "h": ch, "n": npx, "bit_depth": 8}
    chain = tq_util.oracle_encode_batch(oracle, b)
    o = tabs.scan_offset(ts, 0)
    bits = np.array([rate_util.coeff_bits(T[1], chain["qcoeff"][i * npx:(i + 1) * npx], tabs.iscan_pool[o:o + npx], int(chain["eob"][i]), ts, 0,
                                          plane_type=1, is_inter=0) for i in range(n_tu)], np.uint32)
    want = cu.decide_batch(chain["dist"], bits, shift, ab, jobs)
    assert len(set(want["intra_chroma_mode"])) == 2 and len(set(want["cfl_alpha_signs"])) >= 3   # DC and several CfL outcomes

    # the same on the device, nothing read back in between
    d_l, d_cb, d_cr, d_desc = cu.to_dev(luma), cu.to_dev(cb), cu.to_dev(cr), cu.to_dev(desc)
    d_pool = torch.zeros(n_tu * npx, dtype=torch.uint8, device="cuda:0")
    d_src, d_tu, d_qp, d_iscan = cu.to_dev(src.reshape(-1)), cu.to_dev(tu), cu.to_dev(qparams), cu.to_dev(tabs.iscan_pool)
    d_recon = torch.zeros(n_tu * npx, dtype=torch.uint8, device="cuda:0")
    d_q = torch.zeros(n_tu * npx, dtype=torch.int32, device="cuda:0")
    d_eob = torch.zeros(n_tu, dtype=torch.int16, device="cuda:0")
    d_dist = torch.zeros(n_tu * 2, dtype=torch.int64, device="cuda:0")
    d_bits = torch.zeros(n_tu, dtype=torch.int32, device="cuda:0")
    d_tab, d_rd, d_ab, d_job = cu.to_dev(z["tables"]), cu.to_dev(rd), cu.to_dev(ab), cu.to_dev(jobs)
    d_out = torch.zeros(n * cu.DECISION.itemsize, dtype=torch.uint8, device="cuda:0")
    hip_ctx.av1_cfl_alpha_candidates_batch_dev(d_l.data_ptr(), d_cb.data_ptr(), d_cr.data_ptr(), d_desc.data_ptr(), n, lw, lh, d_pool.data_ptr())
    hip_ctx.encode_tu_batch_dev(d_src.data_ptr(), d_pool.data_ptr(), d_recon.data_ptr(), d_tu.data_ptr(), n_tu, cw, ch, d_qp.data_ptr(),
                                d_iscan.data_ptr(), None, d_q.data_ptr(), None, d_eob.data_ptr(), None, d_dist.data_ptr())
    hip_ctx.coeff_rate_batch_dev(d_tab.data_ptr() + svtav1_hip.COEFF_RATE_TABLES_DTYPE.itemsize, d_q.data_ptr(), d_eob.data_ptr(),
                                 d_iscan.data_ptr(), d_rd.data_ptr(), n_tu, ts, d_bits.data_ptr())
    hip_ctx.cfl_alpha_decision_batch_dev(d_dist.data_ptr(), d_bits.data_ptr(), shift, d_ab.data_ptr(), d_job.data_ptr(), n, d_out.data_ptr())
    hip_ctx.synchronize()
    assert np.array_equal(d_pool.cpu().numpy().reshape(pool.shape), pool)
    assert np.array_equal(d_dist.cpu().numpy().view(np.uint64).reshape(n_tu, 2), chain["dist"])
    assert np.array_equal(d_bits.cpu().numpy().view(np.uint32), bits)
    assert np.array_equal(d_out.cpu().numpy().view(cu.DECISION), want)


def test_host_refusals(hip_ctx):
    torch = pytest.importorskip("torch")
    E = svtav1_hip.SvtHipError
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    assert p % 16 == 0
    for (w, h) in ((4, 4), (8, 4), (64, 64), (32, 64), (12, 8), (0, 0), (16, 24)):
        with pytest.raises(E, match="CfL luma size"):
            hip_ctx.av1_cfl_pred_batch_dev(p, p, p, p, p, p, 1, w, h)
        with pytest.raises(E, match="CfL luma size"):
            hip_ctx.av1_highbd_cfl_pred_batch_dev(p, p, p, p, p, p, 1, w, h, 10)
        with pytest.raises(E, match="CfL luma size"):
            hip_ctx.av1_cfl_alpha_candidates_batch_dev(p, p, p, p, 1, w, h, p)
    for miss in range(6):
        args = [None if i == miss else p for i in range(6)]
        with pytest.raises(E, match="null"):
            hip_ctx.av1_cfl_pred_batch_dev(*args, 1, 16, 16)
        with pytest.raises(E, match="null"):
            hip_ctx.av1_highbd_cfl_pred_batch_dev(*args, 1, 16, 16, 10)
    for miss in range(5):
        args = [None if i == miss else p for i in range(5)]
        with pytest.raises(E, match="null"):
            hip_ctx.av1_cfl_alpha_candidates_batch_dev(*args[:4], 1, 16, 16, args[4])
        with pytest.raises(E, match="null"):
            hip_ctx.cfl_alpha_decision_batch_dev(args[0], args[1], 2, args[2], args[3], 1, args[4])
    with pytest.raises(E, match="16-byte"):
        hip_ctx.av1_cfl_pred_batch_dev(p, p, p, p, p, p + 4, 1, 16, 16)
    with pytest.raises(E, match="16-byte"):
        hip_ctx.av1_highbd_cfl_pred_batch_dev(p, p, p, p, p, p + 8, 1, 16, 16, 10)
    with pytest.raises(E, match="16-byte"):
        hip_ctx.av1_cfl_alpha_candidates_batch_dev(p, p, p, p + 4, 1, 16, 16, p)
    with pytest.raises(E, match="16-byte"):
        hip_ctx.cfl_alpha_decision_batch_dev(p, p, 2, p, p + 8, 1, p)
    with pytest.raises(E, match="16-byte"):
        hip_ctx.cfl_alpha_decision_batch_dev(p, p, 2, p, p, 1, p + 8)
    with pytest.raises(E, match="2-byte"):
        hip_ctx.av1_highbd_cfl_pred_batch_dev(p + 1, p, p, p, p, p, 1, 16, 16, 10)
    for bad_bd in (8, 12):
        with pytest.raises(E, match="bit_depth"):
            hip_ctx.av1_highbd_cfl_pred_batch_dev(p, p, p, p, p, p, 1, 16, 16, bad_bd)
    for bad_shift in (64, 1 << 31):
        with pytest.raises(E, match="dist_shift"):
            hip_ctx.cfl_alpha_decision_batch_dev(p, p, bad_shift, p, p, 1, p)
    hip_ctx.av1_cfl_pred_batch_dev(None, None, None, None, None, None, 0, 16, 16)          # n_blocks == 0: OK
    hip_ctx.av1_highbd_cfl_pred_batch_dev(None, None, None, None, None, None, 0, 16, 16, 10)
    hip_ctx.av1_cfl_alpha_candidates_batch_dev(None, None, None, None, 0, 16, 16, None)
    hip_ctx.cfl_alpha_decision_batch_dev(None, None, 2, None, None, 0, None)
    hip_ctx.synchronize()
    assert not buf.cpu().numpy().any()
    assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_device_refusal_leaves_the_destination(hip_ctx, bd):
    pytest.importorskip("torch")
    E = svtav1_hip.SvtHipError
    for (lw, lh) in ((8, 8), (32, 32)):
        n = 23
        luma, cb, cr, desc = cu.random_case(np.random.default_rng(55 + lw), n, lw, lh, bd)
        bad = (0, 5, 6, n - 1)
        desc["alpha_signs"][list(bad)] = (8, 9, 255, 128)
        want_cb, want_cr = cb.copy(), cr.copy()
        assert cu.predict(luma, cb, cr, want_cb, want_cr, desc, lw, lh, bd) == len(bad)
        got_cb, got_cr = cu.run_device(hip_ctx, luma, cb, cr, desc, lw, lh, bd)
        assert np.array_equal(got_cb, want_cb) and np.array_equal(got_cr, want_cr)
        at = np.arange(lh // 2)[:, None] * (lw // 2) + np.arange(lw // 2)[None, :]
        for i in bad:
            assert np.array_equal(got_cb[int(desc[i]["cb_offset"]) + at], cb[int(desc[i]["cb_offset"]) + at])
        with pytest.raises(E, match=f"{len(bad)} PU.*alpha_signs"):
            hip_ctx.inter_pred_refused()
        assert hip_ctx.inter_pred_refused() == 0


def test_caller_stream_without_synchronisation(hip_ctx):
    torch = pytest.importorskip("torch")
    for bd, (lw, lh) in ((8, (8, 8)), (10, (16, 8)), (8, (32, 32)), (10, (8, 32))):
        n = 37
        luma, cb, cr, desc = cu.random_case(np.random.default_rng(70 + lw + lh), n, lw, lh, bd)
        want_cb, want_cr = cb.copy(), cr.copy()
        cu.predict(luma, cb, cr, want_cb, want_cr, desc, lw, lh, bd)
        s = torch.cuda.Stream()
        d_l, d_cb, d_cr, d_desc = cu.to_dev(luma), cu.to_dev(cb), cu.to_dev(cr), cu.to_dev(desc)
        s.wait_stream(torch.cuda.current_stream())   # stream order, not a host wait
        with torch.cuda.stream(s):
            args = (d_l.data_ptr(), d_cb.data_ptr(), d_cr.data_ptr(), d_cb.data_ptr(), d_cr.data_ptr(), d_desc.data_ptr(), n, lw, lh)
            if bd == 8:
                hip_ctx.av1_cfl_pred_batch_dev(*args, stream=s.cuda_stream)
            else:
                hip_ctx.av1_highbd_cfl_pred_batch_dev(*args, 10, stream=s.cuda_stream)
            h_cb, h_cr = d_cb.to("cpu"), d_cr.to("cpu")   # enqueued on s behind the prediction
        view = (lambda t: t.numpy()) if bd == 8 else (lambda t: t.numpy().view(np.uint16))
        assert np.array_equal(view(h_cb), want_cb) and np.array_equal(view(h_cr), want_cr), (bd, lw, lh)
    # candidates and decision on a caller's stream, read back behind them on that stream
    rng = np.random.default_rng(9)
    luma, cb, cr, desc = cu.random_case(rng, 5, 16, 16, 8)
    ab = cu.random_alpha_bits(rng)
    dist, bits, jobs = cu.random_decision_tables(rng, 70)
    d2 = np.zeros((70 * 66, 2), np.uint64)
    d2[:, 0] = dist.reshape(-1)
    s = torch.cuda.Stream()
    d_l, d_cb, d_cr, d_desc = cu.to_dev(luma), cu.to_dev(cb), cu.to_dev(cr), cu.to_dev(desc)
    d_d, d_b, d_a, d_j = cu.to_dev(d2), cu.to_dev(bits.reshape(-1)), cu.to_dev(ab), cu.to_dev(jobs)
    d_pool = torch.zeros(5 * 66 * 64, dtype=torch.uint8, device="cuda:0")
    d_out = torch.zeros(70 * cu.DECISION.itemsize, dtype=torch.uint8, device="cuda:0")
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip_ctx.av1_cfl_alpha_candidates_batch_dev(d_l.data_ptr(), d_cb.data_ptr(), d_cr.data_ptr(), d_desc.data_ptr(), 5, 16, 16, d_pool.data_ptr(),
                                                   stream=s.cuda_stream)
        hip_ctx.cfl_alpha_decision_batch_dev(d_d.data_ptr(), d_b.data_ptr(), 1, d_a.data_ptr(), d_j.data_ptr(), 70, d_out.data_ptr(),
                                             stream=s.cuda_stream)
        h_pool, h_out = d_pool.to("cpu"), d_out.to("cpu")
    assert np.array_equal(h_pool.numpy().reshape(5, 2, 33, 64), cu.candidates(luma, cb, cr, desc, 16, 16))
    assert np.array_equal(h_out.numpy().view(cu.DECISION), cu.decide_batch(dist, bits, 1, ab, jobs))
    assert hip_ctx.inter_pred_refused() == 0
