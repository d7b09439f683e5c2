"""Per-item minima of the 85-PU full-pel search (class forms: search width a multiple of 16): the search loop keeps, per PU, the minimum
SAD of an item (16 consecutive positions of a search row) with the item's first raster index, and three resolver passes after the
search find the first position inside the winning item.  Checked bit for bit against the CPU oracle on inputs where "the first minimum
in raster order" is decided by the parts that are new: equal minima in different quads of an item, in different items of a row, in
different rows (the smaller y must win, whatever lane holds it), and everywhere at once (flat).  The 64x64 PU's 32-bit key
(sum << 12 | y * 64 + x) holds for areas up to 64x64; one taller and one wider area must still give the oracle's result.

The first two tests need no GPU: they show, with the oracle alone (one 1x1 search area per position = the SAD surface of all 85 PUs),
that the inputs really hold ties at the minimum for the 16x16, 32x32 and 64x64 PUs, and that the first tied position in raster
order is what the oracle's search returns."""
import numpy as np
import pytest

import svtav1_hip
from svtav1_hip import synth

W, H = 256, 192
KINDS = ["flat", "two_levels", "three_levels", "period_x4", "period_x8", "period_x16", "period_y4", "period_y16", "period_xy"]
PU_GROUPS = {"64x64": range(0, 1), "32x32": range(1, 5), "16x16": range(5, 21), "8x8": range(21, 85)}


def _pictures(kind, seed=2024):
    """(current, reference).  period_*: the reference repeats exactly in x and / or y, so every PU's SAD surface repeats with it."""
    rng = np.random.default_rng(seed)
    if kind == "flat":
        a = np.full((H, W), 131, np.uint8)
        return synth.PaPicture(a), synth.PaPicture(a.copy())
    if kind in ("two_levels", "three_levels"):
        n = 2 if kind == "two_levels" else 3
        return (synth.PaPicture((rng.integers(0, n, (H, W)) * 90).astype(np.uint8)),
                synth.PaPicture((rng.integers(0, n, (H, W)) * 90).astype(np.uint8)))
    px = {"period_x4": 4, "period_x8": 8, "period_x16": 16, "period_xy": 16}.get(kind, 0)
    py = {"period_y4": 4, "period_y16": 16, "period_xy": 16}.get(kind, 0)
    cell = rng.integers(0, 256, (py or H, px or W), dtype=np.uint8)
    ref = np.tile(cell, (H // cell.shape[0], W // cell.shape[1]))
    cur = rng.integers(0, 256, (H, W), dtype=np.uint8)
    return synth.PaPicture(cur), synth.PaPicture(ref)


def _desc(cur, ref, search, centers=None, inner=False):
    """Descriptors of all superblocks (or, inner: of those whose windows lie wholly inside the picture, where a periodic reference is
    periodic), none of them clipped: the class forms are what runs."""
    nx, ny = cur.sb_grid()
    if centers is None:
        centers = [(0, 0)] * (nx * ny)
    desc = svtav1_hip.make_fullpel_desc(cur, ref, centers, *search)
    assert (desc[:, 4] == search[0]).all() and (desc[:, 5] == search[1]).all(), "a window was clipped"
    if inner:
        keep = [sy * nx + sx for sy in range(ny) for sx in range(nx)
                if 64 * sx + desc[sy * nx + sx, 2] >= 0 and 64 * sx + desc[sy * nx + sx, 2] + search[0] + 63 <= cur.width
                and 64 * sy + desc[sy * nx + sx, 3] >= 0 and 64 * sy + desc[sy * nx + sx, 3] + search[1] + 63 <= cur.height]
        assert keep
        desc = desc[keep]
    return desc


def _sad_surfaces(oracle, cur, ref, d):
    """SADs of the 85 PUs at every position of descriptor d's area, [sh, sw, 85], from the oracle alone: one 1x1 area per position."""
    sw, sh = int(d[4]), int(d[5])
    one = np.empty((sh * sw, 6), np.int32)
    ys, xs = np.divmod(np.arange(sh * sw), sw)
    one[:, 0] = d[0]
    one[:, 1] = d[1] + ys * ref.stride + xs
    one[:, 2] = d[2] + xs
    one[:, 3] = d[3] + ys
    one[:, 4] = 1
    one[:, 5] = 1
    sad, _ = oracle.fullpel_search_batch(cur.full, ref.full, one)
    return sad.reshape(sh, sw, 85)


def _mv_word(x, y):
    return (((y * 4) & 0xffff) << 16) | ((x * 4) & 0xffff)


# which PU sizes must show a tie at the minimum: everywhere for the flat and the periodic pictures (their surfaces repeat inside a
# 64x64 area by construction); random pictures of few levels tie where the number of distinct sums is small against 4096 positions
MUST_TIE = {"flat": ("64x64", "32x32", "16x16", "8x8"), "two_levels": ("16x16", "8x8"), "three_levels": ("16x16", "8x8")}


@pytest.mark.parametrize("kind", KINDS)
def test_inputs_hold_ties_at_the_minimum(oracle, kind):
    cur, ref = _pictures(kind)
    desc = _desc(cur, ref, (64, 64), inner=kind.startswith("period"))
    want_sad, want_mv = oracle.fullpel_search_batch(cur.full, ref.full, desc)
    tied = {g: 0 for g in PU_GROUPS}
    n_pu = {g: 0 for g in PU_GROUPS}
    for i in (0, len(desc) - 1):
        surf = _sad_surfaces(oracle, cur, ref, desc[i])
        for g, pus in PU_GROUPS.items():
            for pu in pus:
                s = surf[:, :, pu]
                at_min = np.argwhere(s == s.min())
                y, x = at_min[0]  # argwhere is in raster order
                assert s.min() == want_sad[i, pu] and _mv_word(int(desc[i, 2]) + int(x), int(desc[i, 3]) + int(y)) == want_mv[i, pu]
                tied[g] += len(at_min) > 1
                n_pu[g] += 1
    print(kind, {g: f"{tied[g]}/{n_pu[g]}" for g in PU_GROUPS})
    everywhere = kind == "flat" or kind.startswith("period")
    for g in MUST_TIE.get(kind, tuple(PU_GROUPS)):
        assert (tied[g] == n_pu[g]) if everywhere else (tied[g] > 0), (kind, g, tied, n_pu)


def test_period_ties_fall_in_the_intended_places(oracle):
    """period 4 in x: the minimum repeats in every quad of an item; period 16: in every item of a row, same place; period in y: in rows
    of different lanes (4) and of different passes of 16 rows (16)."""
    for kind, dx, dy in (("period_x4", 4, 0), ("period_x8", 8, 0), ("period_x16", 16, 0), ("period_y4", 0, 4), ("period_y16", 0, 16),
                         ("period_xy", 16, 16)):
        cur, ref = _pictures(kind)
        desc = _desc(cur, ref, (64, 64), inner=True)
        surf = _sad_surfaces(oracle, cur, ref, desc[0]).astype(np.int64)
        if dx:
            assert np.array_equal(surf[:, dx:], surf[:, :-dx]), kind
        if dy:
            assert np.array_equal(surf[dy:], surf[:-dy]), kind


def _compare(hip_ctx, oracle, cur, ref, desc):
    s_h, m_h = hip_ctx.fullpel_search(cur.full, ref.full, desc)
    s_o, m_o = oracle.fullpel_search_batch(cur.full, ref.full, desc)
    bad = np.argwhere((s_h != s_o) | (m_h != m_o))
    assert bad.size == 0, (f"{len(bad)} mismatches, first (sb,pu)={bad[0]}: hip sad/mv {s_h[tuple(bad[0])]}/{m_h[tuple(bad[0])]:#x} "
                           f"oracle {s_o[tuple(bad[0])]}/{m_o[tuple(bad[0])]:#x}; PUs {sorted(set(bad[:, 1]))[:20]}")


AREAS = [(64, 64), (48, 64), (16, 64), (64, 17), (64, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("search", AREAS)
def test_item_minima_match_oracle(hip_ctx, oracle, kind, search):
    """64-wide areas take the two-image class loop, 48 and 16 the one-image class loop; 17 rows and 1 row leave lanes past the last
    row.  Centres vary per superblock but keep every window unclipped."""
    cur, ref = _pictures(kind)
    rng = np.random.default_rng(search[0] * 131 + search[1])
    nx, ny = cur.sb_grid()
    centers = rng.integers(-20, 21, size=(nx * ny, 2))
    _compare(hip_ctx, oracle, cur, ref, _desc(cur, ref, search, centers))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_item_minima_zero_centres(hip_ctx, oracle, kind):
    """Zero centres: the periodic references are periodic over the whole window of the inner superblocks."""
    cur, ref = _pictures(kind, seed=7)
    _compare(hip_ctx, oracle, cur, ref, _desc(cur, ref, (64, 64)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["two_levels", "period_x4", "period_x16", "period_y4", "period_xy"])
@pytest.mark.parametrize("search", [(64, 64), (48, 64)])
def test_item_minima_every_window_alignment(hip_ctx, oracle, kind, search):
    """Window origins at every byte offset from a 4-byte boundary, in both class loops."""
    cur, ref = _pictures(kind, seed=5)
    nx, ny = cur.sb_grid()
    centers = [(dx, dy) for dy in (0, 3) for dx in range(-3, 5)][:nx * ny]
    desc = _desc(cur, ref, search, centers)
    assert set((desc[:, 1] & 3).tolist()) == {0, 1, 2, 3}
    _compare(hip_ctx, oracle, cur, ref, desc)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["flat", "two_levels", "period_x8", "period_y16"])
@pytest.mark.parametrize("search", [(64, 80), (80, 64)])
def test_areas_above_64_keep_the_two_word_64x64_form(hip_ctx, oracle, kind, search):
    """y * 64 + x does not hold a position of these areas: the 64x64 PU must still be tracked as (SAD, index) pairs there, while the
    smaller PUs use the item minima (both widths are multiples of 16)."""
    cur, ref = _pictures(kind, seed=9)
    rng = np.random.default_rng(3)
    nx, ny = cur.sb_grid()
    centers = rng.integers(-8, 9, size=(nx * ny, 2))
    _compare(hip_ctx, oracle, cur, ref, _desc(cur, ref, search, centers))
