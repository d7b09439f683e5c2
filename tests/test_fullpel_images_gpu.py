"""GPU parity of the two-image form of the 85-PU full-pel search (fullpel85_img2_kernel: launches whose search areas are at most 64x64)
against the CPU oracle, bit for bit.  The cases are the ones its lane -> item map and its second window image make interesting: areas
that fill the last pass of 16 rows partly or with one row, widths below 64 (which keep the one-image loop inside the new kernel), flat
and tie-heavy pictures (a wrong row order shows as a different first minimum), every byte alignment of the window origin, and a search
height above 64, which must still reach the one-image kernel."""
import numpy as np
import pytest

import svtav1_hip
from svtav1_hip import synth

pytestmark = pytest.mark.gpu


def _pictures(w, h, kind, seed=1234):
    rng = np.random.default_rng(seed)
    if kind == "synth":
        return synth.PaPicture(synth.synth_luma(w, h, 1)), synth.PaPicture(synth.synth_luma(w, h, 0))
    if kind == "flat":
        a = np.full((h, w), 77, np.uint8)
        return synth.PaPicture(a), synth.PaPicture(a.copy())
    if kind == "coarse":  # few grey levels: many exact SAD ties at non-trivial positions
        return (synth.PaPicture((rng.integers(0, 3, (h, w)) * 100).astype(np.uint8)),
                synth.PaPicture((rng.integers(0, 3, (h, w)) * 100).astype(np.uint8)))
    return (synth.PaPicture(rng.integers(0, 256, (h, w), dtype=np.uint8)),
            synth.PaPicture(rng.integers(0, 256, (h, w), dtype=np.uint8)))


def _compare(hip_ctx, oracle, cur, ref, desc):
    s_h, m_h = hip_ctx.fullpel_search(cur.full, ref.full, desc)
    s_o, m_o = oracle.fullpel_search_batch(cur.full, ref.full, desc)
    bad = np.argwhere((s_h != s_o) | (m_h != m_o))
    assert bad.size == 0, (f"{len(bad)} mismatches, first (sb,pu)={bad[0]}: hip sad/mv {s_h[tuple(bad[0])]}/{m_h[tuple(bad[0])]:#x} "
                           f"oracle {s_o[tuple(bad[0])]}/{m_o[tuple(bad[0])]:#x}; PUs {sorted(set(bad[:, 1]))[:20]}")


AREAS = [(64, 64), (48, 64), (32, 40), (16, 64), (64, 17), (64, 1)]


@pytest.mark.parametrize("kind", ["synth", "flat", "coarse", "random"])
@pytest.mark.parametrize("search", AREAS)
def test_two_image_areas_match_oracle(hip_ctx, oracle, kind, search):
    """Random centres; 64-wide areas take the two-image loop, the narrower ones the one-image loop inside the same kernel, and the
    heights 40 / 17 / 1 leave the last pass of 16 rows partly empty."""
    cur, ref = _pictures(256, 192, kind)
    rng = np.random.default_rng(search[0] * 131 + search[1])
    nx, ny = cur.sb_grid()
    centers = rng.integers(-40, 41, size=(nx * ny, 2))
    desc = svtav1_hip.make_fullpel_desc(cur, ref, centers, *search)
    assert desc[:, 4].max() <= 64 and desc[:, 5].max() <= 64
    _compare(hip_ctx, oracle, cur, ref, desc)


@pytest.mark.parametrize("kind", ["flat", "coarse"])
def test_two_image_unclipped_64x64_ties(hip_ctx, oracle, kind):
    """Every superblock takes the two-image loop (zero centres on a picture whose padding holds the whole window)."""
    cur, ref = _pictures(320, 256, kind, seed=77)
    desc = svtav1_hip.make_fullpel_desc(cur, ref, None, 64, 64)
    assert (desc[:, 4] == 64).all() and (desc[:, 5] == 64).all()
    _compare(hip_ctx, oracle, cur, ref, desc)


@pytest.mark.parametrize("kind", ["random", "coarse"])
def test_two_image_every_window_alignment(hip_ctx, oracle, kind):
    """Window origins at byte offsets -3 .. 4 from a 4-byte boundary, 64x64 areas: image 1 is image 0 one dword later at each of them."""
    cur, ref = _pictures(512, 128, kind, seed=5)
    nx, ny = cur.sb_grid()
    centers = [(dx, 0) for dx in range(-3, 5)] * ((nx * ny + 7) // 8)
    desc = svtav1_hip.make_fullpel_desc(cur, ref, centers[:nx * ny], 64, 64)
    assert (desc[:, 4] == 64).all()
    assert set((desc[:, 1] & 3).tolist()) == {0, 1, 2, 3}
    _compare(hip_ctx, oracle, cur, ref, desc)


@pytest.mark.parametrize("search", [(64, 65), (64, 100), (80, 64)])
def test_taller_or_wider_areas_keep_the_one_image_kernel(hip_ctx, oracle, search):
    """Above 64 in either direction the launch goes to fullpel85_kernel as before."""
    cur, ref = _pictures(256, 192, "coarse", seed=9)
    rng = np.random.default_rng(3)
    nx, ny = cur.sb_grid()
    centers = rng.integers(-20, 21, size=(nx * ny, 2))
    desc = svtav1_hip.make_fullpel_desc(cur, ref, centers, *search)
    assert max(desc[:, 4].max(), desc[:, 5].max()) > 64
    _compare(hip_ctx, oracle, cur, ref, desc)
