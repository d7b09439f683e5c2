"""CPU: the numpy restatement of AV1 intra prediction (tests/intra_pred_util.py) reproduces the reference's fixture
(tests/golden/intra_pred.npz) bit for bit and, where the reference sources and oracle/_ref/obj_all exist, a live run of the reference on
random cases.  The reference has no PAETH predictor (pred[PAETH_PRED] is never assigned, Codec/EbIntraPrediction.c:6907-), so the fixture
and the live run cover its 12 modes, and PAETH is held to the AV1 specification's rule (7.11.2.2) instead: on hand-worked samples and on
the vectors of tests/paeth_vectors.py, which are worked sample by sample in code that shares nothing with the restatement."""
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import intra_pred_util as iu  # noqa: E402
import make_golden_intra_pred as mg  # noqa: E402
import paeth_vectors as pv  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "intra_pred.npz")


def fixture_cases():
    g = np.load(GOLDEN)
    desc = g["desc"].view(iu.DESC)
    out = []
    for (ts, bd, d0, dn, e0, en, o0, on) in g["case"]:
        out.append((int(ts), int(bd), g[f"edge_{bd}"][e0:e0 + en], desc[d0:d0 + dn], g[f"out_{bd}"][o0:o0 + on]))
    return out, g["pos"], g["md"], g["md_out"]


def test_restatement_matches_fixture():
    cases, _, _, _ = fixture_cases()
    n = 0
    for (ts, bd, edge, desc, want) in cases:
        txw, txh = iu.TX_SIZES_WH[ts]
        dst = np.full(len(desc) * txw * txh, iu.FILL[bd], edge.dtype)
        refused, _ = iu.predict(edge, dst, desc, ts, bd)
        assert refused == 0
        bad = np.flatnonzero(dst != want)
        assert bad.size == 0, (ts, bd, bad[:4] // (txw * txh), desc[bad[0] // (txw * txh)])
        n += len(desc)
    assert n >= 2000


def test_fixture_covers_the_ground():
    cases, pos, md, md_out = fixture_cases()
    assert mg.coverage([(ts, bd, edge, desc) for (ts, bd, edge, desc, _) in cases]) is None
    # blocks whose counts the reference derived at picture positions, through its 8-bit and its 16-bit caller, some of them cut by the
    # right / bottom picture edge
    for bd in (8, 10):
        mine = [p for p in pos if cases[p[0]][1] == bd]
        assert len(mine) >= 300
        assert sum(1 for (_, _, w, h, _, x, y) in mine if x + w > mg.PIC_W or y + h > mg.PIC_H) >= 20
        assert {int(cases[p[0]][3][p[1]]["mode"]) for p in mine} == {m for m, _ in mg.POSITION_MODES}
    # the mode-decision sequence gave the EncDec block for the same position, counts and mode
    assert len(md) >= 40
    o = 0
    for (row, i) in md:
        ts, bd, _, _, want = cases[row]
        w, h = iu.TX_SIZES_WH[ts]
        assert bd == 8 and np.array_equal(md_out[o:o + w * h], want[i * w * h:(i + 1) * w * h]), (row, i)
        o += w * h
    assert o == len(md_out)


@pytest.mark.parametrize("bd", [8, 10])
def test_paeth_vectors(bd):
    for ts in pv.SIZES:
        edge, desc, want, winners = pv.vectors(ts, bd)
        assert winners == {"left", "top", "topleft"}, (ts, bd)
        st = iu.new_stats()
        dst = np.zeros(len(want), edge.dtype)
        assert iu.predict(edge, dst, desc, ts, bd, stats=st)[0] == 0
        assert np.array_equal(dst, want), (ts, bd)
        assert st["paeth"] == winners
    if bd == 10:
        assert max(int(pv.vectors(ts, 10)[2].max()) for ts in pv.SIZES) == 1023


def test_paeth_follows_the_specification():
    # base = top + left - topleft; the candidate nearest to base wins, ties to left, then top
    for (top, left, tl, want) in ((100, 50, 60, 100),   # base 90: |90-50| 40, |90-100| 10, |90-60| 30 -> top
                                  (50, 100, 60, 100),   # base 90 -> left
                                  (100, 50, 75, 75),    # base 75 -> topleft
                                  (80, 80, 80, 80), (0, 255, 255, 0), (255, 0, 0, 255)):
        a = np.array([tl, top, top, top, top, 0, 0, 0, 0], np.int64)
        lf = np.array([tl, left, left, left, left, 0, 0, 0, 0], np.int64)
        st = iu.new_stats()
        out = iu.predict_from_edges(a, lf, iu.PAETH, 0, 4, 4, True, True, 8, st)
        assert (out == want).all(), (top, left, tl)


def test_sad_is_the_plain_sum():
    rng = np.random.default_rng(5)
    for ts in (0, 2, 18):
        txw, txh = iu.TX_SIZES_WH[ts]
        edge, desc, src = iu.random_case(rng, 9, ts, 8)
        dst = np.zeros(9 * txw * txh, np.uint8)
        _, sad = iu.predict(edge, dst, desc, ts, 8, src=src)
        want = np.abs(dst.astype(np.int64) - src.astype(np.int64)).reshape(9, -1).sum(axis=1)
        assert np.array_equal(sad, want)


def test_refusals_of_the_restatement():
    d = np.zeros(1, iu.DESC)[0]
    for field, value in (("mode", 13), ("angle_delta", 4), ("angle_delta", -4), ("n_top_px", 9), ("n_left_px", 5), ("n_topright_px", 9)):
        b = d.copy()
        b["n_top_px"], b["n_left_px"] = 8, 4
        b[field] = value
        assert not iu.desc_valid(b, 8, 4)
    b = d.copy()
    b["n_top_px"], b["n_topright_px"] = 7, 1
    assert not iu.desc_valid(b, 8, 4)
    b = d.copy()
    b["n_left_px"], b["n_bottomleft_px"] = 3, 1
    assert not iu.desc_valid(b, 8, 4)


@pytest.mark.skipif(not mg.reference_available(), reason="needs the reference sources and oracle/_ref/obj_all")
def test_restatement_matches_live_reference():
    rng = np.random.default_rng(20261017)
    total = 0
    with tempfile.TemporaryDirectory() as tmp:
        L = mg.build_driver(tmp)
        for bd in (8, 10):
            for ts, (w, h) in enumerate(iu.TX_SIZES_WH):
                n = 150 if w * h <= 256 else 60 if w * h <= 1024 else 20
                edge, desc, _ = iu.random_case(rng, n, ts, bd, n_modes=12)
                want = mg.reference_blocks(L, edge, desc, ts, bd).reshape(-1)
                dst = np.zeros(n * w * h, edge.dtype)
                assert iu.predict(edge, dst, desc, ts, bd)[0] == 0
                bad = np.flatnonzero(dst != want)
                assert bad.size == 0, (ts, bd, desc[bad[0] // (w * h)])
                total += n
    assert total >= 3000
