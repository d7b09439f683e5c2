"""8x8 PUs of the 85-PU full-pel search's class forms: an item's sixteen raw SADs are reduced with v_pk_minimum3_f16, which is an exact
packed u16 minimum only while every value is the bit pattern of a non-negative finite f16 (raw 8x8 SAD <= 8160 = 0x1fe0 < 0x7c00) and
only if the hardware passes denormals (1..1023) through unchanged; the two-image form (search width 64) then keeps one running packed
minimum of 4 * sad + pass per PU instead of a key per pass, and stages its window with a routine fixed to that width.  The tie rules
are pinned by test_fullpel_item_minima_gpu.py; the inputs here are chosen by the RANGE of the 8x8 SADs instead, and compared bit for
bit with the CPU oracle:

  levels4         both pictures uniform random in 100..103: every 8x8 SAD of the surface is <= 96, all f16 denormals;
  levels160       uniform random in 40..199: the surface and the winners straddle 0x03ff / 0x0400, denormal against normal operands
                  (an amplitude of 40 leaves the whole surface below 700 and the winners at 191..301, so it is 160 here);
  full            uniform random in 0..255, the normal range;
  white_on_black  current picture 255, reference 0: every 8x8 SAD is 8160, the top of the range, all tied: the first position wins;
  spots           the same with 600 reference pixels raised by 1..120: minima just below 8160.

The first test needs no GPU: it shows with the oracle alone that the winners lie where the list above says."""
import functools

import numpy as np
import pytest

import svtav1_hip
from svtav1_hip import synth

W, H = 256, 192
KINDS = ["levels4", "levels160", "full", "white_on_black", "spots"]
AREAS = [(64, 64), (64, 33), (64, 17), (64, 1), (48, 64)]
SEED = 2025


@functools.lru_cache(maxsize=None)
def _pictures(kind):
    rng = np.random.default_rng(SEED)
    if kind in ("levels4", "levels160", "full"):
        lo, hi = {"levels4": (100, 104), "levels160": (40, 200), "full": (0, 256)}[kind]
        cur, ref = rng.integers(lo, hi, (H, W)).astype(np.uint8), rng.integers(lo, hi, (H, W)).astype(np.uint8)
    else:
        cur, ref = np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8)
        if kind == "spots":
            ref[rng.integers(0, H, 600), rng.integers(0, W, 600)] = rng.integers(1, 121, 600)
    return synth.PaPicture(cur), synth.PaPicture(ref)


def _desc(cur, ref, search, centers=None):
    desc = svtav1_hip.make_fullpel_desc(cur, ref, centers, *search)
    assert (desc[:, 4] == search[0]).all() and (desc[:, 5] == search[1]).all(), "a window was clipped"
    return desc


def _mv_word(x, y):
    return (((y * 4) & 0xffff) << 16) | ((x * 4) & 0xffff)


def test_inputs_lie_in_their_sad_ranges(oracle):
    """Winning raw 8x8 SADs (sad / 2 of PUs 21..84) of every superblock at a 64x64 area."""
    raw, mv, desc = {}, {}, {}
    for kind in KINDS:
        cur, ref = _pictures(kind)
        desc[kind] = _desc(cur, ref, (64, 64))
        sad, mv[kind] = oracle.fullpel_search_batch(cur.full, ref.full, desc[kind])
        assert (sad[:, 21:] % 2 == 0).all()
        raw[kind] = sad[:, 21:] // 2
        print(kind, "winning raw 8x8 SADs", raw[kind].min(), "..", raw[kind].max(), "distinct", len(np.unique(raw[kind])))
    r = raw["levels4"]
    assert r.min() >= 1 and r.max() <= 1023 and len(np.unique(r)) >= 8
    r = raw["levels160"]
    assert (r < 1024).any() and (r >= 1024).any()
    assert (raw["white_on_black"] == 8160).all()
    d = desc["white_on_black"]
    first = np.array([_mv_word(int(x), int(y)) for x, y in d[:, 2:4]], np.uint32)
    assert (mv["white_on_black"][:, 21:] == first[:, None]).all(), "all tied: the area's first position must win"
    r = raw["spots"]
    assert r.min() >= 7000 and r.max() <= 8159


def _compare(hip_ctx, oracle, cur, ref, desc):
    s_h, m_h = hip_ctx.fullpel_search(cur.full, ref.full, desc)
    s_o, m_o = oracle.fullpel_search_batch(cur.full, ref.full, desc)
    bad = np.argwhere((s_h != s_o) | (m_h != m_o))
    assert bad.size == 0, (f"{len(bad)} mismatches, first (sb,pu)={bad[0]}: hip sad/mv {s_h[tuple(bad[0])]}/{m_h[tuple(bad[0])]:#x} "
                           f"oracle {s_o[tuple(bad[0])]}/{m_o[tuple(bad[0])]:#x}; PUs {sorted(set(bad[:, 1]))[:20]}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("search", AREAS)
def test_tagged_minima_match_oracle(hip_ctx, oracle, kind, search):
    """64-wide areas take the two-image form (tags, minimum3, fixed-shape staging) with four full passes (64 rows), a partial third
    (33), a partial second (17) and a partial first one (1); 48-wide areas the one-image class form (minimum3 with a key per pass)."""
    cur, ref = _pictures(kind)
    _compare(hip_ctx, oracle, cur, ref, _desc(cur, ref, search))


@pytest.mark.gpu
@pytest.mark.parametrize("search", [(64, 64), (64, 33)])
def test_fixed_shape_staging_at_every_window_alignment(hip_ctx, oracle, search):
    """Per-superblock centres in -20..20: the window origins take every byte offset from a 4-byte boundary."""
    cur, ref = _pictures("full")
    nx, ny = cur.sb_grid()
    centers = np.random.default_rng(SEED + search[1]).integers(-20, 21, size=(nx * ny, 2))
    desc = _desc(cur, ref, search, centers)
    assert set((desc[:, 1] & 3).tolist()) == {0, 1, 2, 3}
    _compare(hip_ctx, oracle, cur, ref, desc)
