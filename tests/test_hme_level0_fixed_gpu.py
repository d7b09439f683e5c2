"""GPU parity of the one-band, fixed-shape form of HME level 0 (wave_sad_loop_l0_oneband in me_hme_impl.h): full SBs whose clipped
level-0 width is a multiple of 16 and whose window fits the wave's LDS slice in one band.  Descriptors and centres are compared bit
for bit with the oracle for every SB of list 0, with the checking pattern of tests/test_hme_shapes_gpu.py.

What the new form changes is how an item's raster base and window address are stepped from pass to pass, how the 16 keys of an item are
formed (relative to the item, base added once) and how the window rows reach LDS (one 16-byte store per load).  The inputs are chosen
so that a wrong step, base or row shows:
  * 640 x 384 (10 x 6 SBs, the 576p-or-lower class: 48 x 40 regions at 200 %, three items per row, one whole pass and two remainder
    rounds) with synthetic, flat (ties everywhere) and x- / y-periodic content (ties inside an item, between items, between rows);
    once with level 0 alone, so that its centre reaches the descriptor without two more searches that might cover a wrong one;
  * 1200 x 576 (19 x 9 SBs, the smallest size of the 1080p class: 96 x 48 regions at 200 %, six items per row, four whole passes
    and a 32-item remainder: the headline's level-0 shape) with synthetic, flat and x-periodic content, and with a reference that is the current picture
    shifted by a multiple of four samples, so that the 1/16 planes are exact shifts and level 0's minimum is an exact match.  The
    shift puts the match of one SB on the positions where the new indexing can go wrong.  640 x 384 cannot hold these targets: it is
    in the class whose regions are 48 wide (nit = 3, no item 256), it has no partial SB, and a clipped width that is not a multiple of
    16 appears there only where the centre check moves a window.  1200 x 576 is the nearest size that has all of them.

The first tests need no GPU: they restate the centre check and level 0's window clipping on the host and show that the inputs take the
paths they are meant to take (the new form for at least a quarter of the (SB, region) pairs, each fallback at least once, every
shifted match on its target position of a window that takes the new form)."""
import numpy as np
import pytest

import svtav1_hip
from svtav1_hip import synth

SMALL = (640, 384)
LARGE = (1200, 576)
LDS_PER_WAVE = 7 * 1024   # kHmeLdsPerWave


def _periodic_pics(w, h, px, py):
    """(current, reference): the reference repeats exactly every px samples in x or py in y (one of them 0: no period there)."""
    rng = np.random.default_rng(2025)
    cell = rng.integers(0, 256, (py or h, px or w), dtype=np.uint8)
    ref = np.tile(cell, (h // cell.shape[0], w // cell.shape[1]))
    cur = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return [synth.PaPicture(cur), synth.PaPicture(ref), synth.PaPicture(ref)]


def _shifted_pics(w, h, dx, dy):
    """(current, reference) with reference(p + 4 * (dx, dy)) == current(p): (dx, dy) is the displacement on the 1/16 plane."""
    mx, my = 416, 224   # beyond the largest level-0 displacement of the 1080p class at 200 % (96 + 15, 48 + 15 on the 1/16 plane)
    big = synth.synth_luma(w + 2 * mx, h + 2 * my, 0)
    cur = big[my:my + h, mx:mx + w]
    ref = big[my - 4 * dy:my - 4 * dy + h, mx - 4 * dx:mx - 4 * dx + w]
    ref = synth.PaPicture(np.ascontiguousarray(ref))
    return [synth.PaPicture(np.ascontiguousarray(cur)), ref, ref]


def _pics(w, h, kind):
    if kind == "period_x":
        return _periodic_pics(w, h, 16, 0)    # period 4 on the 1/16 plane: ties inside an item and between items
    if kind == "period_y":
        return _periodic_pics(w, h, 0, 16)    # period 4 in rows: ties between search rows
    from test_hme_gpu import _pics as chain_pics
    return chain_pics(w, h, kind)


def _clamp_center(x, y, ox, oy, pw, ph):
    x = (-63 - ox) if ox + x < -63 else x
    x = (x - ((ox + x) - (pw - 1))) if ox + x > pw - 1 else x
    y = (-63 - oy) if oy + y < -63 else y
    y = (y - ((oy + y) - (ph - 1))) if oy + y > ph - 1 else y
    return x, y


def _clip_window(xo, yo, sw, sh, ox, oy, padw, padh, pw, ph):
    """The four statements per axis of me_hme_impl.h's clip_window, each re-reading what the previous wrote."""
    xo = (-padw - ox) if ox + xo < -padw else xo
    sw = (sw - (-padw - (ox + xo))) if ox + xo < -padw else sw
    xo = (xo - ((ox + xo) - (pw - 1))) if ox + xo > pw - 1 else xo
    sw = max(1, sw - ((ox + xo + sw) - pw)) if ox + xo + sw > pw else sw
    yo = (-padh - oy) if oy + yo < -padh else yo
    sh = (sh - (-padh - (oy + yo))) if oy + yo < -padh else sh
    yo = (yo - ((oy + yo) - (ph - 1))) if oy + yo > ph - 1 else yo
    sh = max(1, sh - ((oy + yo + sh) - ph)) if oy + yo + sh > ph else sh
    return xo, yo, sw, sh


def _centre_check(cur, ref, P, ox, oy):
    """hme_mv_center_check of a full SB, list 0: candidates 0 / B / C / D on the 64 x 32-row block, first minimum in that order."""
    tw, th = P.hme_level0_total_search_area_width, P.hme_level0_total_search_area_height
    pad = synth.PAD_FULL
    src = cur.full[pad + oy:pad + oy + 64:2, pad + ox:pad + ox + 64].astype(np.int64)
    best = None
    for x, y in ((0, 0), (tw, 0), (0, -th), (0, th)):
        cx, cy = _clamp_center(x, y, ox, oy, ref.width, ref.height)
        blk = ref.full[pad + oy + cy:pad + oy + cy + 64:2, pad + ox + cx:pad + ox + cx + 64].astype(np.int64)
        sad = int(np.abs(src - blk).sum())
        if best is None or sad < best[0]:
            best = (sad, x, y)
    return best[1], best[2]


def _level0_windows(pics, P):
    """{(sb index, region): (kind, xo, yo, sw, sh)} of list 0; kind is "fixed" (the new form), "width" (not a multiple of 16), "bands"
    (more than one band or more than 65536 positions) or "partial" (the SB is not 64 x 64: general loop, or no HME at all)."""
    cur, ref = pics[0], pics[1]
    mx, my = P.hme_level0_multiplier_x, P.hme_level0_multiplier_y
    tw, th = P.hme_level0_total_search_area_width, P.hme_level0_total_search_area_height
    aw = [P.hme_level0_search_area_in_width_array[k] * mx // 100 for k in range(2)]
    ah = [P.hme_level0_search_area_in_height_array[k] * my // 100 for k in range(2)]
    out = {}
    for i, (ox, oy) in enumerate(svtav1_hip.sb_origins(cur.width, cur.height).astype(int)):
        full = min(64, cur.width - ox) == 64 and min(64, cur.height - oy) == 64
        xc, yc = _centre_check(cur, ref, P, ox, oy) if full else (0, 0)
        for wave in range(4):
            rw, rh = wave % 2, wave // 2
            xo = -((tw * mx // 100) >> 1) + (xc >> 2) + sum(aw[:rw])
            yo = -((th * my // 100) >> 1) + (yc >> 2) + sum(ah[:rh])
            xo, yo, sw, sh = _clip_window(xo, yo, aw[rw], ah[rh], ox >> 2, oy >> 2, 15, 15, ref.width >> 2, ref.height >> 2)
            pitch = 4 * ((sw + 15) >> 4) + 4
            one_band = (LDS_PER_WAVE // 4) // pitch - 14 >= sh and sw * sh <= 65536
            kind = "partial" if not full else "width" if sw & 15 else "fixed" if one_band else "bands"
            out[(i, wave)] = (kind, xo, yo, sw, sh)
    return out


def _params(size, level0_only=False):
    P = svtav1_hip.default_me_params(size[0], size[1], 3, 0)   # hierarchy 3, temporal layer 0: the 200 % level-0 area
    if level0_only:
        P.enable_hme_level1_flag = P.enable_hme_level2_flag = 0
    return P


# Shifted-reference targets at LARGE: (name, SB index, region wave, position (px, py) of the match in the region's 96 x 48 window).
# nit = 6 items per row: item 256 (the first of the remainder passes) is row 42, column item 4; the last item is row 47, item 5.
# The SBs are ones whose centre check keeps the zero centre with the shifted reference, so that the window is where the shift assumes
# it (test_shifted_matches_land_on_their_targets shows it); region 3's window of these SBs is unclipped.
TARGETS = [
    ("first position", 42, 3, 0, 0),
    ("last position of the last row", 42, 3, 95, 47),
    ("position 15 of a row", 42, 3, 15, 5),
    ("position 16 of a row", 42, 3, 16, 5),
    ("first row of the remainder passes", 2, 3, 64, 42),
    ("last item", 45, 3, 80, 47),
]


def _target_shift(target):
    """The 1/16-plane displacement that puts the match of the target's SB on the target's position, with the zero centre the check of
    that SB is shown to pick (test_shifted_matches_land_on_their_targets)."""
    _, sbi, wave, px, py = target
    flat = [synth.PaPicture(np.zeros((LARGE[1], LARGE[0]), np.uint8))] * 2   # a flat picture keeps the zero centre
    _, xo, yo, sw, sh = _level0_windows(flat, _params(LARGE))[(sbi, wave)]
    assert (sw, sh) == (96, 48)
    return xo + px, yo + py


def test_inputs_take_the_new_form_and_each_fallback():
    got = {}
    for size in (SMALL, LARGE):
        kinds = [v[0] for v in _level0_windows(_pics(size[0], size[1], "synth"), _params(size)).values()]
        got[size] = {k: kinds.count(k) for k in ("fixed", "width", "bands", "partial")}
        print(size, got[size])
        assert 4 * got[size]["fixed"] >= len(kinds), got
    # 640 x 384 has no partial SB and, with 48-wide regions on a 160-wide plane, no clipped width that is not a multiple of 16 unless
    # the centre check moves a window; 1200 x 576 has both fallbacks
    assert got[LARGE]["width"] > 0 and got[LARGE]["partial"] > 0, got


@pytest.mark.parametrize("target", TARGETS, ids=[t[0].replace(" ", "_") for t in TARGETS])
def test_shifted_matches_land_on_their_targets(oracle, target):
    """Host and oracle only: the SB's window takes the new form, the match is on the target position, and level 0 alone finds it."""
    name, sbi, wave, px, py = target
    dx, dy = _target_shift(target)
    pics = _shifted_pics(LARGE[0], LARGE[1], dx, dy)
    P = _params(LARGE, level0_only=True)
    kind, xo, yo, sw, sh = _level0_windows(pics, P)[(sbi, wave)]
    assert kind == "fixed" and (sw, sh) == (96, 48) and (dx - xo, dy - yo) == (px, py), (name, kind, xo, yo, sw, sh)
    ox, oy = (int(v) for v in svtav1_hip.sb_origins(*LARGE)[sbi])
    assert 0 <= (ox >> 2) + dx and (ox >> 2) + dx + 16 <= LARGE[0] >> 2 and 0 <= (oy >> 2) + dy and (oy >> 2) + dy + 16 <= LARGE[1] >> 2
    pool, descs = svtav1_hip.build_picture_pool(pics)
    sb = svtav1_hip.sb_origins(*LARGE)
    _, centre = oracle.hme_search_center_batch(pool, descs[0], descs[1], P, 0, sb, None, np.zeros((sb.shape[0], 25), np.int16))
    assert tuple(int(v) for v in centre[sbi]) == (4 * dx, 4 * dy), (name, centre[sbi])


def _run(hip_ctx, oracle, pics, P):
    from test_hme_shapes_gpu import _run_and_check
    return _run_and_check(hip_ctx, oracle, pics, P, False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["synth", "flat", "period_x", "period_y"])
def test_level0_fixed_small_matches_oracle(hip_ctx, oracle, kind):
    pytest.importorskip("torch")
    _run(hip_ctx, oracle, _pics(SMALL[0], SMALL[1], kind), _params(SMALL))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["synth", "period_x"])
def test_level0_alone_matches_oracle(hip_ctx, oracle, kind):
    pytest.importorskip("torch")
    _run(hip_ctx, oracle, _pics(SMALL[0], SMALL[1], kind), _params(SMALL, level0_only=True))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["synth", "flat", "period_x"])
def test_level0_fixed_large_matches_oracle(hip_ctx, oracle, kind):
    """Four stepped passes and the remainder; flat and period_x tie across the passes, so the first item in raster order must win."""
    pytest.importorskip("torch")
    _run(hip_ctx, oracle, _pics(LARGE[0], LARGE[1], kind), _params(LARGE))


@pytest.mark.gpu
@pytest.mark.parametrize("level0_only", [False, True], ids=["all_levels", "level0_alone"])
@pytest.mark.parametrize("target", TARGETS, ids=[t[0].replace(" ", "_") for t in TARGETS])
def test_level0_fixed_shifted_reference_matches_oracle(hip_ctx, oracle, target, level0_only):
    pytest.importorskip("torch")
    dx, dy = _target_shift(target)
    dev = _run(hip_ctx, oracle, _shifted_pics(LARGE[0], LARGE[1], dx, dy), _params(LARGE, level0_only))
    if level0_only:
        assert tuple(int(v) for v in dev[0][1][target[1]]) == (4 * dx, 4 * dy)
