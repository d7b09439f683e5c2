"""RD transform-type search through the batcher (svthip_tu_batcher_set_tx_search / _add_tx_search / _tx_search_result): every TU's
winner, full cost, coefficient bits, eob and distortion equal the serial loop of ProductFullLoopTxSearch (Codec/EbFullLoop.c:1138-1352)
restated on top of the oracle's fused chain (tq_util.oracle_encode_batch) and the rate restatement (rate_util)."""
import numpy as np
import pytest

import rate_util
import svtav1_hip
from tq_util import RealTables, oracle_encode_batch

pytestmark = pytest.mark.gpu
PIC_W, PIC_H = 256, 128


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _golden_tables():
    z = np.load(rate_util.os.path.join(rate_util.ROOT, "tests", "golden", "coeff_rate.npz"))
    return z["tables"].view(svtav1_hip.COEFF_RATE_TABLES_DTYPE).reshape(-1)


def _partition():
    """a 256x128 picture in TUs of all 19 sizes: 64x64, 64x16 / 16x64, 32x32, 2:1 and 4:1 rectangles, 4x4"""
    tus = []

    def tile(ts, x0, y0, w, h):
        tw, th = svtav1_hip.TX_SIZES_WH[ts]
        tus.extend((ts, x, y) for y in range(y0, y0 + h, th) for x in range(x0, x0 + w, tw))

    tile(4, 0, 0, 64, 64)
    tile(18, 64, 0, 64, 64)
    tile(11, 128, 0, 64, 64)
    tile(12, 192, 0, 64, 64)
    tile(3, 0, 64, 32, 32); tile(2, 32, 64, 32, 32); tile(1, 0, 96, 32, 32); tile(0, 32, 96, 32, 32)
    tile(9, 64, 64, 32, 32); tile(10, 96, 64, 32, 32); tile(15, 64, 96, 32, 32); tile(16, 96, 96, 32, 32)
    tile(8, 128, 64, 32, 32); tile(7, 160, 64, 32, 32); tile(6, 128, 96, 32, 32); tile(5, 160, 96, 32, 32)
    tile(17, 192, 64, 32, 64); tile(14, 224, 64, 32, 32); tile(13, 224, 96, 32, 32)
    return tus


def _picture(rng, bit_depth):
    sc = 1 << (bit_depth - 8)
    yy, xx = np.mgrid[0:PIC_H, 0:PIC_W]
    src = np.clip(sc * (128 + 70 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.normal(0, 6, (PIC_H, PIC_W))), 0, 256 * sc - 1)
    pred = np.clip(src + sc * (rng.laplace(0, 7, (PIC_H, PIC_W)) + 10 * np.sin(yy / 3.0)), 0, 256 * sc - 1)
    dt = np.uint8 if bit_depth == 8 else np.uint16
    src, pred = src.astype(dt), pred.astype(dt)
    pred[64:80, 32:48] = src[64:80, 32:48]   # the first 16x16 TU at (32, 64): all-zero residual
    return src, pred


def _tu_params(rng, i, ts):
    inter = int(i % 5 != 3)
    red, fast = int(i % 7 == 5), int(i % 4 == 1)
    return dict(is_inter=inter, intra_mode=int(rng.integers(0, 13)), reduced_tx_set=red, fast=fast,
                type_mask=rate_util.tx_search_type_mask(ts, inter, red, fast), txb_skip_ctx=int(rng.integers(0, 13)),
                dc_sign_ctx=int(rng.integers(0, 3)), lam=int(rng.integers(1000, 400000)), qi=int(rng.integers(0, 3)))


def serial_search(oracle, src, pred, qrows, tables, tabs, bit_depth, ts, x, y, p):
    """ProductFullLoopTxSearch for one TU: every candidate through the oracle chain, its rate, then the decision loop"""
    w, h = svtav1_hip.TX_SIZES_WH[ts]
    n = min(w, 32) * min(h, 32)
    cands, qco = {}, {}
    for tt in range(16):
        if not p["type_mask"] >> tt & 1:
            continue
        d = np.zeros(1, dtype=svtav1_hip.TU_DESC_DTYPE)
        d["src_offset"] = d["pred_offset"] = d["recon_offset"] = y * PIC_W + x
        d["src_stride"] = d["pred_stride"] = d["recon_stride"] = PIC_W
        d["iscan_offset"] = tabs.scan_offset(ts, tt); d["qparam_index"] = p["qi"]; d["tx_type"] = tt
        o = oracle_encode_batch(oracle, {"src": src.reshape(-1), "pred": pred.reshape(-1), "desc": d, "qparams": qrows, "scan": tabs.scan_pool,
                                         "w": w, "h": h, "n": n, "bit_depth": bit_depth})
        eob = int(o["eob"][0])
        so = tabs.scan_offset(ts, tt)
        bits = rate_util.coeff_bits(tables, o["qcoeff"], tabs.iscan_pool[so:so + n], eob, ts, tt, 0, p["txb_skip_ctx"], p["dc_sign_ctx"],
                                    p["is_inter"], p["intra_mode"], p["reduced_tx_set"])
        cands[tt] = (eob, int(o["energy"][0]), int(o["dist"][0, 0]), int(o["dist"][0, 1]), bits)
        qco[tt] = o["qcoeff"]
    return rate_util.decide(ts, p["lam"], cands), cands, qco


def _search(hip_ctx, bat, tus, params, d_tables, tabs):
    bat.set_tx_search(d_tables, [[tabs.scan_offset(ts, tt) for tt in range(16)] for ts in range(19)])
    hs = []
    for (ts, x, y), p in zip(tus, params):
        hs.append(bat.add_tx_search(lambda_=p["lam"], src_offset=y * PIC_W + x, src_stride=PIC_W, pred_offset=y * PIC_W + x, pred_stride=PIC_W,
                                    qparam_index=p["qi"], type_mask=p["type_mask"], tx_size=ts, is_inter=p["is_inter"], intra_mode=p["intra_mode"],
                                    reduced_tx_set=p["reduced_tx_set"], txb_skip_ctx=p["txb_skip_ctx"], dc_sign_ctx=p["dc_sign_ctx"]))
    return hs


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_search_matches_serial_loop(hip_ctx, oracle, bit_depth):
    pytest.importorskip("torch")
    rng = np.random.default_rng(31 + bit_depth)
    tabs = RealTables()
    T = _golden_tables()
    tables = T[1]
    d_tables = _dev(T[1:2])
    src, pred = _picture(rng, bit_depth)
    qrows = np.ascontiguousarray(tabs.rows(bit_depth, "inter")[[30, 90, 160], 0, :])
    tus = _partition()
    params = [_tu_params(rng, i, ts) for i, (ts, _, _) in enumerate(tus)]
    for (ts, _, _), p in zip(tus, params):
        w, h = svtav1_hip.TX_SIZES_WH[ts]
        assert all(t in svtav1_hip.valid_tx_types(w, h) for t in range(16) if p["type_mask"] >> t & 1)
    d_src, d_pred, d_qp, d_iscan = _dev(src), _dev(pred), _dev(qrows), _dev(tabs.iscan_pool)
    bat = svtav1_hip.TuBatcher(hip_ctx, 8192, 1 << 21)
    bat.begin(d_src.data_ptr(), d_pred.data_ptr(), None, bit_depth != 8, d_qp.data_ptr(), d_iscan.data_ptr())
    hs = _search(hip_ctx, bat, tus, params, d_tables.data_ptr(), tabs)
    bat.flush()
    n_rate_matters = n_zero = n_intra = n_fast = 0
    for i, ((ts, x, y), p) in enumerate(zip(tus, params)):
        want, cands, qco = serial_search(oracle, src, pred, qrows, tables, tabs, bit_depth, ts, x, y, p)
        r = bat.tx_search_result(hs[i])
        got = (r.tx_type, r.full_cost, r.coeff_bits, r.eob, r.distortion[0], r.distortion[1])
        assert got == (want["tx_type"], want["full_cost"], want["coeff_bits"], want["eob"], *want["distortion"]), (i, ts, p, cands)
        cr = bat.result(r.candidate)
        assert (cr.tx_size, cr.tx_type, cr.eob) == (ts, r.tx_type, r.eob)
        if i % 9 == 0:
            w, h = svtav1_hip.TX_SIZES_WH[ts]
            q, _ = bat.read_coeffs(r.candidate, min(w, 32) * min(h, 32))
            assert np.array_equal(q, qco[r.tx_type])
        eligible = {t: c for t, c in cands.items() if c[0] or t == 0}
        by_dist = min(eligible, key=lambda t: eligible[t][2])
        n_rate_matters += by_dist != r.tx_type
        if all(c[0] == 0 for c in cands.values()):
            n_zero += 1
            assert r.tx_type == 0 and r.coeff_bits == int(tables["coeffFacBits"][(rate_util.SQR[ts] + rate_util.SQR_UP[ts] + 1) >> 1, 0]
                                                                 ["txb_skip_cost"][p["txb_skip_ctx"], 1])
        n_intra += not p["is_inter"]
        n_fast += p["fast"] and p["type_mask"] != rate_util.tx_search_type_mask(ts, p["is_inter"], p["reduced_tx_set"], 0)
    assert n_rate_matters > 0, "the RD decision never differed from the distortion-only argmin"
    assert n_zero >= 1 and n_intra > 10 and n_fast > 5
    bat.close()


def test_tie_keeps_the_lower_type(hip_ctx, oracle):
    """ADST_DCT and FLIPADST_DCT of a residual that is symmetric top-to-bottom have the same levels and distortion; with equal
    transform-type rates the costs tie exactly and strict '<' keeps ADST_DCT"""
    pytest.importorskip("torch")
    tabs = RealTables()
    arr = _golden_tables()[2:3].copy()
    arr["interTxTypeFacBits"] = 700
    tables = arr[0]
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, (PIC_H, PIC_W)).astype(np.uint8)
    src[8:16] = src[0:8][::-1]
    pred = np.full((PIC_H, PIC_W), 128, np.uint8)
    qrows = np.ascontiguousarray(tabs.rows(8, "inter")[[40], 0, :])
    tus = [(2, x, 0) for x in range(0, 128, 16)]           # 16x16 TUs, rows 0..15 mirrored
    params = [dict(is_inter=1, intra_mode=0, reduced_tx_set=0, fast=0, type_mask=(1 << 1) | (1 << 4), txb_skip_ctx=3, dc_sign_ctx=1,
                   lam=50000, qi=0) for _ in tus]
    assert tabs.scan_offset(2, 1) == tabs.scan_offset(2, 4) or np.array_equal(
        tabs.iscan_pool[tabs.scan_offset(2, 1):][:256], tabs.iscan_pool[tabs.scan_offset(2, 4):][:256])
    bat = svtav1_hip.TuBatcher(hip_ctx, 64, 1 << 14)
    d_src, d_pred, d_qp, d_iscan = _dev(src), _dev(pred), _dev(qrows), _dev(tabs.iscan_pool)
    d_tables = _dev(arr)
    bat.begin(d_src.data_ptr(), d_pred.data_ptr(), None, False, d_qp.data_ptr(), d_iscan.data_ptr())
    hs = _search(hip_ctx, bat, tus, params, d_tables.data_ptr(), tabs)
    bat.flush()
    for h_, (ts, x, y), p in zip(hs, tus, params):
        want, cands, _ = serial_search(oracle, src, pred, qrows, tables, tabs, 8, ts, x, y, p)
        assert cands[1] == cands[4] and cands[1][0] > 0
        r = bat.tx_search_result(h_)
        assert r.tx_type == 1 == want["tx_type"] and r.full_cost == want["full_cost"]
    bat.close()


def test_stale_cost_without_dct(hip_ctx, oracle):
    """a caller mask without DCT_DCT on an all-zero residual: every candidate has eob 0 and is skipped (TX_TYPE_FIX), so the loop
    compares the initial yFullCost = MAX_CU_COST and the first type visited wins with it -- the reference's outcome"""
    pytest.importorskip("torch")
    tabs = RealTables()
    tables = _golden_tables()[0]
    src = np.full((PIC_H, PIC_W), 90, np.uint8)
    pred = src.copy()
    pred[:, 128:] += 40                                     # right half: a real residual, the normal rule applies
    qrows = np.ascontiguousarray(tabs.rows(8, "inter")[[100], 0, :])
    tus = [(1, 0, 0), (1, 64, 8), (1, 128, 0), (1, 192, 16)]
    params = [dict(is_inter=1, intra_mode=0, reduced_tx_set=0, fast=0, type_mask=(1 << 3) | (1 << 9), txb_skip_ctx=5, dc_sign_ctx=0,
                   lam=30000, qi=0) for _ in tus]
    bat = svtav1_hip.TuBatcher(hip_ctx, 64, 1 << 14)
    d_src, d_pred, d_qp, d_iscan = _dev(src), _dev(pred), _dev(qrows), _dev(tabs.iscan_pool)
    d_tables = _dev(_golden_tables()[0:1])
    bat.begin(d_src.data_ptr(), d_pred.data_ptr(), None, False, d_qp.data_ptr(), d_iscan.data_ptr())
    hs = _search(hip_ctx, bat, tus, params, d_tables.data_ptr(), tabs)
    bat.flush()
    for k, (h_, (ts, x, y), p) in enumerate(zip(hs, tus, params)):
        want, cands, _ = serial_search(oracle, src, pred, qrows, tables, tabs, 8, ts, x, y, p)
        r = bat.tx_search_result(h_)
        assert (r.tx_type, r.full_cost, r.coeff_bits, r.eob, tuple(r.distortion)) == (want["tx_type"], want["full_cost"], want["coeff_bits"],
                                                                             want["eob"], want["distortion"])
        if k < 2:
            assert all(c[0] == 0 for c in cands.values())
            assert r.tx_type == 3 and r.full_cost == rate_util.MAX_CU_COST and bat.result(r.candidate).tx_type == 3
        else:
            assert r.full_cost < rate_util.MAX_CU_COST
    bat.close()


def test_mixed_batch_keeps_add_results(hip_ctx):
    """_add candidates flushed together with search TUs return exactly what they return in a flush of their own"""
    pytest.importorskip("torch")
    rng = np.random.default_rng(8)
    tabs = RealTables()
    src, pred = _picture(rng, 8)
    qrows = np.ascontiguousarray(tabs.rows(8, "inter")[[60, 140, 200], 0, :])
    d_src, d_pred, d_qp, d_iscan = _dev(src), _dev(pred), _dev(qrows), _dev(tabs.iscan_pool)
    d_tables = _dev(_golden_tables()[0:1])
    adds = [(ts, tt, x, y) for (ts, x, y) in _partition()[::3] for tt in (0, 9) if tt in svtav1_hip.valid_tx_types(*svtav1_hip.TX_SIZES_WH[ts])]

    def run(with_search):
        bat = svtav1_hip.TuBatcher(hip_ctx, 8192, 1 << 21)
        bat.begin(d_src.data_ptr(), d_pred.data_ptr(), None, False, d_qp.data_ptr(), d_iscan.data_ptr())
        if with_search:
            tus = _partition()[1::2]
            _search(hip_ctx, bat, tus, [_tu_params(rng, i, ts) for i, (ts, _, _) in enumerate(tus)], d_tables.data_ptr(), tabs)
        hs = [bat.add(ts, tt, y * PIC_W + x, PIC_W, y * PIC_W + x, PIC_W, svtav1_hip.TU_RECON_SCRATCH, 0, 1, tabs.scan_offset(ts, tt))
              for ts, tt, x, y in adds]
        bat.flush()
        out = []
        for h_, (ts, tt, _, _) in zip(hs, adds):
            r = bat.result(h_)
            w, hh = svtav1_hip.TX_SIZES_WH[ts]
            q, dq = bat.read_coeffs(h_, min(w, 32) * min(hh, 32))
            out.append((r.eob, r.three_quad_energy, r.distortion[0], r.distortion[1], r.tx_size, r.tx_type, q.tobytes(), dq.tobytes()))
        bat.close()
        return out

    assert run(False) == run(True)


def test_search_refusals(hip_ctx):
    torch = pytest.importorskip("torch")
    tabs = RealTables()
    buf = torch.zeros(1 << 18, dtype=torch.uint8, device="cuda:0")
    d_tables = _dev(_golden_tables()[0:1])
    offs = [[tabs.scan_offset(ts, tt) for tt in range(16)] for ts in range(19)]
    tu = dict(lambda_=1000, src_offset=0, src_stride=64, pred_offset=0, pred_stride=64, qparam_index=0, type_mask=0x0201, tx_size=1, is_inter=1)
    bat = svtav1_hip.TuBatcher(hip_ctx, 4, 4096)
    bat.begin(buf.data_ptr(), buf.data_ptr(), None, False, buf.data_ptr(), buf.data_ptr())
    with pytest.raises(svtav1_hip.SvtHipError):
        bat.add_tx_search(**tu)                                       # before set_tx_search
    bat.set_tx_search(d_tables.data_ptr(), offs)
    with pytest.raises(svtav1_hip.SvtHipError):
        bat.add_tx_search(**dict(tu, type_mask=0))                    # empty mask
    with pytest.raises(svtav1_hip.SvtHipError):
        bat.add_tx_search(**dict(tu, tx_size=19))                     # no such TxSize
    h0 = bat.add_tx_search(**tu)                                      # 2 candidates
    with pytest.raises(svtav1_hip.SvtHipError):
        bat.add_tx_search(**dict(tu, type_mask=0x0e0f))               # 7 more candidates: over the capacity of 4
    with pytest.raises(svtav1_hip.SvtHipError):
        bat.tx_search_result(h0)                                      # not flushed yet
    bat.flush()
    assert bat.tx_search_result(h0).tx_type in (0, 9)
    with pytest.raises(svtav1_hip.SvtHipError):
        bat.tx_search_result(h0 + 1)                                  # no such TU
    bat.close()
