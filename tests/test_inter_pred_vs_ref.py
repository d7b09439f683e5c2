"""Pins the numpy restatement of av1_inter_prediction (tests/inter_pred_util.py) against the reference's own av1_inter_prediction /
av1_inter_prediction_hbd: through the committed fixture tests/golden/inter_pred.npz everywhere, and re-derived live where the reference and
oracle/_ref exist.  Also checks what the fixture covers and that the whole-PU entries are declared and exported.  CPU only."""
import os
import re
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import inter_pred_util as ipu  # noqa: E402
import svtav1_hip  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "inter_pred.npz")
NEW_SYMBOLS = ("svthip_av1_inter_pred_batch_dev", "svthip_av1_highbd_inter_pred_batch_dev", "svthip_inter_pred_refused")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def fixture_refs(g, bd):
    from make_golden_inter_pred import reference_pictures
    return reference_pictures(bd)


def fixture_cases(g):
    for i in range(len(g["case_bw"])):
        s, n = int(g["case_start"][i]), int(g["case_count"][i])
        yield i, int(g["case_bw"][i]), int(g["case_bh"][i]), int(g["case_bd"][i]), g["desc"][s:s + n].view(svtav1_hip.INTER_PU_DESC_DTYPE)


def empty_pred(bd, pic):
    from make_golden_inter_pred import FILL
    dt = np.uint8 if bd == 8 else np.uint16
    return ipu.Picture(np.full((pic, pic), FILL[bd], dt), np.full((pic // 2, pic // 2), FILL[bd], dt), np.full((pic // 2, pic // 2), FILL[bd], dt), 0)


def test_restatement_reproduces_fixture(golden):
    from make_golden_inter_pred import PIC
    refs = {bd: fixture_refs(golden, bd) for bd in (8, 10)}
    for i, bw, bh, bd, desc in fixture_cases(golden):
        pred = empty_pred(bd, PIC)
        assert ipu.predict(refs[bd][0], refs[bd][1], pred, desc, bw, bh, bd) == 0
        for p in ("y", "cb", "cr"):
            want = golden[f"pred_{p}_{bd}"][int(golden["case_pred"][i])]
            bad = np.argwhere(getattr(pred, p) != want)
            assert bad.size == 0, (i, (bw, bh, bd), p, bad[:4])


def test_fixture_covers_the_ground(golden):
    desc = golden["desc"].view(svtav1_hip.INTER_PU_DESC_DTYPE)
    per = [(bw, bh, bd, d) for _, bw, bh, bd, d in fixture_cases(golden)]
    assert {(bw, bh) for bw, bh, _, _ in per} == set(ipu.SIZES)
    assert {bd for _, _, bd, _ in per} == {8, 10}
    assert set(desc["pred_direction"].tolist()) == {0, 1, 2}
    assert {(int(f) >> 16, int(f) & 0xffff) for f in desc["interp_filters"]} == {(x, y) for x in range(4) for y in range(4)}
    # every intra / inter mix of each sub-8x8 neighbourhood, uni-predicted and going sub-8x8 where the mix is all inter
    for bd in (8, 10):
        for (bw, bh) in ipu.SUB8_SIZES:
            used = [k for k in range(3) if (k == 0 and bw == 4 and bh == 4) or (k == 1 and bh == 4) or (k == 2 and bw == 4)]
            mixes = set()
            n_sub8 = 0
            for w, h, b, ds in per:
                if (w, h, b) != (bw, bh, bd):
                    continue
                for d in ds:
                    if d["has_uv"] and d["pred_direction"] != 2:
                        mixes.add(tuple(int(d["nb_is_inter"][k]) for k in used))
                        n_sub8 += ipu.sub8x8(d, bw, bh)
            assert len(mixes) == 1 << len(used), (bw, bh, bd, mixes)
            assert n_sub8 > 0
    # vectors clamped on each of the four edges (luma clamp)
    hit = set()
    for bw, bh, _, ds in per:
        for d in ds:
            for l in range(2):
                r, c = ipu.clamp_mv(d, d["mv"][l][0], d["mv"][l][1], bw, bh, 0)
                if c != ipu._i16(2 * int(d["mv"][l][1])):
                    hit.add("left" if c < 0 else "right")
                if r != ipu._i16(2 * int(d["mv"][l][0])):
                    hit.add("top" if r < 0 else "bottom")
    assert hit == {"left", "right", "top", "bottom"}
    # a sub-8x8 piece whose neighbour takes list 1 (ref_frame[0] not LAST_FRAME), and an own piece on list 1 with a list-0 direction
    assert any(ipu.sub8x8(d, bw, bh) and any(d["nb_is_inter"][k] and d["nb_list"][k] for k in range(3)) for bw, bh, _, ds in per for d in ds)
    assert any(ipu.sub8x8(d, bw, bh) and d["pred_direction"] == 0 and d["own_list"] == 1 for bw, bh, _, ds in per for d in ds)


def test_restatement_rederived_live_against_reference():
    import make_golden_inter_pred as mg
    if not mg.reference_available():
        pytest.skip("the reference sources / oracle/_ref are not on this machine")
    rng = np.random.default_rng(77)
    with tempfile.TemporaryDirectory() as tmp:
        L = mg.build_driver(tmp)
        for bd in (8, 10):
            refs = mg.reference_pictures(bd)
            for (bw, bh) in ipu.SIZES:
                desc = ipu.random_descs(rng, min(6, (mg.PIC // bw) * (mg.PIC // bh)), bw, bh, mg.PIC, mg.PIC, clamp_frac=0.3)
                rft = mg.ref_frame_types(L, rng, desc)
                want, got = empty_pred(bd, mg.PIC), empty_pred(bd, mg.PIC)
                mg.reference_predict(L, refs, want, desc, rft, bw, bh, bd)
                assert ipu.predict(refs[0], refs[1], got, desc, bw, bh, bd) == 0
                for p in ("y", "cb", "cr"):
                    assert np.array_equal(getattr(got, p), getattr(want, p)), ((bw, bh, bd), p)


def test_inter_pred_symbols_declared_and_exported():
    with open(os.path.join(ROOT, "include", "svtav1_hip.h")) as f:
        declared = set(re.findall(r"\b(svthip_\w+)\s*\(", f.read()))
    lib = svtav1_hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert svtav1_hip.INTER_PU_DESC_DTYPE.itemsize == 64
