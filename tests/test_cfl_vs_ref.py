"""The numpy restatement of chroma-from-luma prediction and of cfl_rd_pick_alpha's walk (tests/cfl_util.py) bit for bit against what the
reference's own functions wrote and decided (tests/golden/cfl.npz, made by tests/golden/make_golden_cfl.py), the fixture's coverage, and a
live run of fresh cases where the reference exists."""
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import cfl_util as cu  # noqa: E402
import make_golden_cfl as mg  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "cfl.npz")


def fixture_cases(g=None):
    """[(lw, lh, bd, luma, cb, cr, desc, want_cb, want_cr, ac)]"""
    g = np.load(GOLDEN) if g is None else g
    desc_all = g["desc"].view(cu.DESC)
    out = []
    for (lw, lh, bd, d0, dn, l0, ln, c0, cn, a0, an) in g["case"]:
        sl, sc = slice(l0, l0 + ln), slice(c0, c0 + cn)
        out.append((int(lw), int(lh), int(bd), g[f"luma_{bd}"][sl], g[f"cb_{bd}"][sc], g[f"cr_{bd}"][sc], desc_all[d0:d0 + dn],
                    g[f"ocb_{bd}"][sc], g[f"ocr_{bd}"][sc], g["ac"][a0:a0 + an]))
    return out


def fixture_decisions(g=None):
    g = np.load(GOLDEN) if g is None else g
    return (g["dec_alpha_bits"], g["dec_group"], g["dec_dist"], g["dec_bits"], g["dec_job"].view(cu.JOB), g["dec_out"], g["dec_mask"],
            int(g["dec_dist_shift"][0]))


def test_restatement_matches_fixture():
    n = 0
    for (lw, lh, bd, luma, cb, cr, desc, want_cb, want_cr, want_ac) in fixture_cases():
        got_cb, got_cr = cb.copy(), cr.copy()
        assert cu.predict(luma, cb, cr, got_cb, got_cr, desc, lw, lh, bd) == 0
        assert np.array_equal(got_cb, want_cb) and np.array_equal(got_cr, want_cr), (lw, lh, bd)
        ac = np.concatenate([cu.block_ac(luma, d, lw, lh, bd).reshape(-1) for d in desc])
        assert np.array_equal(ac, want_ac), (lw, lh, bd)
        # in place gives the same: a block's DC prediction is read before it is overwritten
        assert cu.predict(luma, got_cb := cb.copy(), got_cr := cr.copy(), got_cb, got_cr, desc, lw, lh, bd) == 0
        assert np.array_equal(got_cb, want_cb) and np.array_equal(got_cr, want_cr)
        n += len(desc)
    assert n >= 18 * 14


def test_idx_to_alpha_matches_fixture():
    rows = np.load(GOLDEN)["alpha"]
    assert len(rows) == 256 * 8 * 2
    for (idx, js, plane, want) in rows:
        assert cu.idx_to_alpha(int(idx), int(js), int(plane)) == want
    for a_u in range(-16, 17):
        for a_v in range(-16, 17):
            if a_u or a_v:
                idx, js = cu.alpha_to_fields(a_u, a_v)
                assert (cu.idx_to_alpha(idx, js, 0), cu.idx_to_alpha(idx, js, 1)) == (a_u, a_v)


def test_fixture_covers_the_ground():
    ab, group, dist, bits, jobs, _, _, shift = fixture_decisions()
    assert shift == mg.DIST_SHIFT
    cases = [(lw, lh, bd, luma, cb, cr, desc) for (lw, lh, bd, luma, cb, cr, desc, _, _, _) in fixture_cases()]
    assert mg.coverage(cases, ab, group, dist, bits, jobs) is None
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "intra_pred.npz"))


def test_decision_restatement_matches_the_reference_walk():
    """outcome and evaluated alphas as the reference's own cfl_rd_pick_alpha produced them on the fixture's tables"""
    ab, group, dist, bits, jobs, want_out, want_mask, shift = fixture_decisions()
    for g in range(len(ab)):
        sel = np.flatnonzero(group == g)
        got = cu.decide_batch(dist[sel], bits[sel], shift, ab[g], jobs[sel])
        for i, o in zip(sel, got):
            assert (o["intra_chroma_mode"], o["cfl_alpha_idx"], o["cfl_alpha_signs"]) == tuple(want_out[i]), (i, o, want_out[i])
            assert tuple(o["evaluated_mask"]) == tuple(want_mask[i]), (i, o, want_mask[i])
    # what the reference never evaluates: Cr with alpha -1 (AV1CostCalcCfl predicts with alpha 0 where both alpha fields are 0)
    assert not (want_mask[:, 1] & np.uint64(1 << 15)).any() and (want_mask[:, 0] & np.uint64(1 << 15)).all()
    assert (want_mask & np.uint64(1 << 16)).all()


def test_candidates_outside_the_mask_do_not_matter():
    ab, group, dist, bits, jobs, _, _, shift = fixture_decisions()
    sel = np.flatnonzero(group == 0)
    got = cu.decide_batch(dist[sel], bits[sel], shift, ab[0], jobs[sel])
    d2, b2 = dist[sel].copy(), bits[sel].copy()
    k = np.arange(33, dtype=np.uint64)
    for i, o in enumerate(got):
        for p in range(2):
            out = ((np.uint64(o["evaluated_mask"][p]) >> k) & np.uint64(1)) == 0
            d2[i, p, out] = (1 << 62) - 1   # large, yet RDCOST of it stays below 2^63 only if never formed: the restatement asserts that
            b2[i, p, out] = 0xffffffff
    again = cu.decide_batch(d2, b2, shift, ab[0], jobs[sel])
    assert np.array_equal(got, again)


def test_refusal_of_the_restatement():
    luma, cb, cr, desc = cu.random_case(np.random.default_rng(3), 4, 16, 16, 8)
    desc["alpha_signs"][2] = 8
    ocb, ocr = cb.copy(), cr.copy()
    assert cu.predict(luma, cb, cr, ocb, ocr, desc, 16, 16, 8) == 1
    at = int(desc[2]["cb_offset"]) + np.arange(8)[:, None] * int(desc[2]["chroma_stride"]) + np.arange(8)[None, :]
    assert np.array_equal(ocb[at], cb[at])


def test_candidates_are_predictions():
    rng = np.random.default_rng(11)
    luma, cb, cr, desc = cu.random_case(rng, 3, 16, 8, 8)
    pool = cu.candidates(luma, cb, cr, desc, 16, 8)
    for k in (0, 15, 16, 17, 32):
        d = desc.copy()
        for i in range(3):
            d[i]["alpha_idx"], d[i]["alpha_signs"] = cu.alpha_to_fields(k - 16, k - 16) if k != 16 else cu.alpha_to_fields(0, 1)
        ocb, ocr = cb.copy(), cr.copy()
        cu.predict(luma, cb, cr, ocb, ocr, d, 16, 8, 8)
        at = np.arange(4)[:, None] * 8 + np.arange(8)[None, :]
        for i in range(3):
            assert np.array_equal(pool[i, 0, k].reshape(4, 8), ocb[int(d[i]["cb_offset"]) + at])
            if k != 16:
                assert np.array_equal(pool[i, 1, k].reshape(4, 8), ocr[int(d[i]["cr_offset"]) + at])


@pytest.mark.skipif(not mg.reference_available(), reason="needs the reference sources and oracle/_ref/obj_all")
def test_restatement_matches_live_reference():
    rng = np.random.default_rng(20261019)
    with tempfile.TemporaryDirectory() as tmp:
        L = mg.build_driver(tmp)
        for bd in (8, 10):
            for (lw, lh) in cu.LUMA_SIZES_WH:
                luma, cb, cr, desc = cu.random_case(rng, 9, lw, lh, bd, chroma_pad=16 - lw // 2)
                want_cb, want_cr, _ = mg.reference_predict(L, luma, cb, cr, desc, lw, lh, bd)
                got_cb, got_cr = cb.copy(), cr.copy()
                cu.predict(luma, cb, cr, got_cb, got_cr, desc, lw, lh, bd)
                assert np.array_equal(got_cb, want_cb) and np.array_equal(got_cr, want_cr), (lw, lh, bd)
        ab = cu.random_alpha_bits(rng)
        dist, bits, jobs = cu.random_decision_tables(rng, 120)
        got = cu.decide_batch(dist, bits, 2, ab, jobs)
        for i in range(len(jobs)):
            out, masks = mg.reference_decide(L, dist[i] >> np.uint64(2), bits[i], ab, jobs[i])
            assert (got[i]["intra_chroma_mode"], got[i]["cfl_alpha_idx"], got[i]["cfl_alpha_signs"]) == tuple(out), i
            assert tuple(got[i]["evaluated_mask"]) == tuple(masks), i
