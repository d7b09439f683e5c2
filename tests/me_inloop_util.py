"""TEST INFRASTRUCTURE -- numpy restatement of the in-loop motion estimation the library builds (include/svtav1_hip.h, "In-loop motion
estimation"): centres, search areas, the full-pel search of the 849 blocks of a 64x64 superblock and the reorder into inloop_me_mv, with the
case list and the picture builders of tests/golden/inloop_me.npz.  Nothing here is shared with the kernels: the block table is built from
the rule (z-order of the enclosing square, then the place along the shorter side), the SADs from an integral image over the 4x4 leaves."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "inloop_me.npz")

N_BLOCKS = 849
MAX_SAD_VALUE = 128 * 128 * 255
BORDER = 64          # what the header states for the full-pel search: the window reaches 63 samples beyond the picture each way
# (w, h, first slot) of the 19 runs of p_sb_best_sad / p_sb_best_mv (Codec/EbProductCodingLoop.c:6346-6363)
SHAPES = [(4, 4, 0), (8, 8, 256), (16, 16, 320), (32, 32, 336), (64, 64, 340), (8, 4, 341), (4, 8, 469), (4, 16, 597), (16, 4, 661), (16, 8, 725),
          (8, 16, 757), (32, 8, 789), (8, 32, 805), (32, 16, 821), (16, 32, 829), (64, 16, 837), (16, 64, 841), (64, 32, 845), (32, 64, 847)]
SIDE_4_SHAPES = {(4, 4), (8, 4), (4, 8), (16, 4), (4, 16)}


def zorder(bx, by):
    return sum(((bx >> i) & 1) << (2 * i) | ((by >> i) & 1) << (2 * i + 1) for i in range(4))


def slot_in_shape(w, h, x, y):
    q = max(w, h)
    return zorder(x // q, y // q) * (q * q // (w * h)) + ((y % q) // h if w > h else (x % q) // w)


def block_table():
    """(blocks [849][4] = x, y, w, h of every buffer slot; pack_source [849] = the buffer slot candidate c of inloop_me_mv reads;
    side_4 [849] bool)"""
    blocks = np.zeros((N_BLOCKS, 4), np.int32)
    source = np.zeros(N_BLOCKS, np.int32)
    side4 = np.zeros(N_BLOCKS, bool)
    seen = np.zeros(N_BLOCKS, bool)
    for w, h, start in SHAPES:
        cols = 64 // w
        for r in range(cols * (64 // h)):   # raster within the shape: the candidate order of :6635-6727
            x, y = (r % cols) * w, (r // cols) * h
            slot = start + slot_in_shape(w, h, x, y)
            assert not seen[slot]
            seen[slot] = True
            blocks[slot] = (x, y, w, h)
            source[start + r] = slot
            side4[slot] = (w, h) in SIDE_4_SHAPES
    # The reference's tab4x16 (:3005-3010) is not the inverse of its walk: raster candidate (col, row) of the 4x16 run reads the 16x16 unit
    # (row & 1) | (col >> 2) << 1 | (row >> 1) << 3 instead of the z-order unit (col >> 2 & 1) | (row & 1) << 1 | (col >> 3) << 2 | (row >> 1) << 3,
    # so 32 of the 64 candidates carry the vector of another 4x16 block.  inloop_me_mv is what mode decision reads: reproduced.
    r = np.arange(64)
    col, row = r % 16, r // 16
    source[597:661] = 597 + 4 * ((row & 1) | (col >> 2) << 1 | (row >> 1) << 3) + (col & 3)
    assert seen.all()
    return blocks, source, side4


BLOCKS, PACK_SOURCE, SIDE_4 = block_table()


def permutation_tables():
    """{shape name: raster -> buffer order inside the shape's run}: what the reference stores as tab4x4, tab8x4, ... tab32x64"""
    out = {}
    for i, (w, h, start) in enumerate(SHAPES):
        n = (SHAPES[i + 1][2] if i + 1 < len(SHAPES) else N_BLOCKS) - start
        out[f"{w}x{h}"] = PACK_SOURCE[start:start + n] - start
    return out


def sb_origins(width, height):
    return np.array([(x, y) for y in range(0, height, 64) for x in range(0, width, 64)], np.int32)


def centers(me_rows, list_index):
    """me_rows: structured [n_sb][stride] with xMvL0 .. yMvL1 -> int16 [n_sb][2] (Codec/EbEncDecProcess.c:1558-1563)"""
    k = ("xMvL1", "yMvL1") if list_index else ("xMvL0", "yMvL0")
    return np.stack([me_rows[k[0]][:, 0] >> 2, me_rows[k[1]][:, 0] >> 2], axis=1).astype(np.int16)


def _axis(center, area, origin, pic):
    """one axis of :6389-6446, statement by statement"""
    pad = 63
    size = min(area, 127)
    o = center - (size >> 1)
    o = -pad - origin if origin + o < -pad else o
    size = size - (-pad - (origin + o)) if origin + o < -pad else size
    o = o - ((origin + o) - (pic - 1)) if origin + o > pic - 1 else o
    size = max(1, size - ((origin + o + size) - pic)) if origin + o + size > pic else size
    return o, size


def area(center, sbs, width, height, src_geom, ref_geom, area_w, area_h):
    """-> int32 [n_sb][8] = svthip_inloop_desc; src_geom / ref_geom = (stride, origin_x, origin_y)"""
    out = np.zeros((len(sbs), 8), np.int32)
    for i, (sx, sy) in enumerate(sbs):
        xo, sw = _axis(int(center[i][0]), area_w, int(sx), width)
        yo, sh = _axis(int(center[i][1]), area_h, int(sy), height)
        out[i] = ((src_geom[2] + sy) * src_geom[0] + src_geom[1] + sx, (ref_geom[2] + sy + yo) * ref_geom[0] + ref_geom[1] + sx + xo, xo, yo, sw, sh,
                  min(width - sx, 64), min(height - sy, 64))
    return out


def fullpel_sb(src_plane, src_stride, ref_plane, ref_stride, d):
    """one superblock: (best_sad [849], best_mv [849]) uint32, buffer order.  src_plane / ref_plane flat uint8"""
    so, ro, xo, yo, sw, sh, bw, bh = (int(v) for v in d)
    src = np.zeros((64, 64), np.int16)
    src[:bh, :bw] = np.lib.stride_tricks.as_strided(src_plane[so:], (bh, bw), (src_stride, 1))
    win = np.lib.stride_tricks.as_strided(ref_plane[ro:], (sh + 63, sw + 63), (ref_stride, 1)).astype(np.int16)
    x0, y0 = BLOCKS[:, 0] // 4, BLOCKS[:, 1] // 4
    x1, y1 = x0 + BLOCKS[:, 2] // 4, y0 + BLOCKS[:, 3] // 4
    sads = np.zeros((N_BLOCKS, sh, sw), np.uint32)
    for py in range(sh):
        v = np.lib.stride_tricks.sliding_window_view(win[py:py + 64], 64, axis=1)           # [64 rows][sw][64]
        leaf = np.abs(v - src[:, None, :]).astype(np.uint32).reshape(16, 4, sw, 16, 4).sum(axis=(1, 4))   # [ly][sw][lx]
        integral = np.zeros((17, sw, 17), np.uint32)
        integral[1:, :, 1:] = leaf.cumsum(axis=0).cumsum(axis=2)
        sads[:, py, :] = integral[y1, :, x1] - integral[y0, :, x1] - integral[y1, :, x0] + integral[y0, :, x0]
    flat = sads.reshape(N_BLOCKS, sh * sw)
    pos = flat.argmin(axis=1)                     # the first minimum in raster order: strict '<' from MAX_SAD_VALUE
    best = flat[np.arange(N_BLOCKS), pos]
    assert best.max() < MAX_SAD_VALUE
    mx, my = xo + pos % sw, yo + pos // sw
    mv = (((my * 4) & 0xFFFF).astype(np.uint32) << 16) | ((mx * 4) & 0xFFFF).astype(np.uint32)   # :3619-3621
    return best.astype(np.uint32), mv


def fullpel(src_plane, src_stride, ref_plane, ref_stride, desc):
    r = [fullpel_sb(src_plane, src_stride, ref_plane, ref_stride, d) for d in desc]
    return np.stack([a for a, _ in r]), np.stack([b for _, b in r])


def pack(best_mv):
    """[n][849] uint32 -> int16 [n][849][2], x then y, candidate order (:6626-6728)"""
    m = best_mv[:, PACK_SOURCE]
    return np.stack([(m & 0xFFFF).astype(np.uint16).view(np.int16), (m >> 16).astype(np.uint16).view(np.int16)], axis=2)


# ------------------------------------------------------------------------------------------------ cases

def pad_plane(pic, border=BORDER):
    return np.pad(pic, border, mode="edge")


def _random_pair(rng, w, h):
    return rng.integers(0, 256, (h, w), dtype=np.uint8), [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(2)]


def _texture(w, h, phase):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return 128 + 60 * np.sin((x + phase[0]) * 0.37) * np.cos((y + phase[1]) * 0.23) + 40 * np.sin((x + phase[0]) * 0.11 + (y + phase[1]) * 0.17)


def make_cases():
    """[(name, src [h][w], [ref per list], centers int16 [lists][n_sb][2], area_w, area_h)].  136x72: two full SB columns and one 8 wide, a
    full SB row and one 8 high."""
    rng = np.random.default_rng(20261020)
    cases = []
    src, refs = _random_pair(rng, 136, 72)
    # centres (x, y) per SB and list: the left and top clip arms beyond -63 (list 0, SBs 0 and 3; SB 5), widths the right clip leaves no multiple
    # of 4 (list 0, SBs 1 and 2), the bottom arms (the SB row at y = 64, 8 rows high), origins pulled back to the last column / row with
    # MAX(1, ..) leaving an area 1 wide (list 1, SBs 2 and 5) and one 1 high (list 1, SBs 4 and 5).  The generator asserts the arms.
    c0 = [(-100, -90), (43, -10), (5, 3), (-70, 20), (0, 0), (-3, -120)]
    c1 = [(0, 0), (43, 12), (90, -40), (10, 5), (3, 200), (300, 300)]
    cases.append(("random", src, refs, np.array([c0, c1], np.int16), 64, 64))
    s1, r1 = _random_pair(rng, 64, 64)
    cases.append(("small_odd", s1, r1[:1], np.array([[(3, -2)]], np.int16), 21, 13))
    cases.append(("largest", s1, r1[1:], np.array([[(0, 0)]], np.int16), 127, 127))
    cases.append(("flat", np.full((72, 136), 90, np.uint8), [np.full((72, 136), 97, np.uint8)] * 2, np.zeros((2, 6, 2), np.int16), 64, 64))
    cases.append(("extreme", np.zeros((64, 64), np.uint8), [np.full((64, 64), 255, np.uint8)], np.zeros((1, 1, 2), np.int16), 64, 64))
    # a reference equal to the source shifted by (+1.5, -0.25) samples
    t = np.clip(np.rint(_texture(136, 72, (0, 0))), 0, 255).astype(np.uint8)
    ts = [np.clip(np.rint(_texture(136, 72, (1.5, -0.25))), 0, 255).astype(np.uint8), np.clip(np.rint(_texture(136, 72, (-2.5, 3.25))), 0, 255).astype(np.uint8)]
    cases.append(("shifted", t, ts, np.zeros((2, 6, 2), np.int16), 64, 64))
    return cases


def restate_case(src, refs, ctr, area_w, area_h, use_subpel=False, trace=None):
    """{desc [lists][n_sb][8], best_sad, best_mv [lists][n_sb][849], inloop_mv [lists][n_sb][849][2]} on planes built the way the tests build
    them: the source unpadded, the references padded by BORDER"""
    h, w = src.shape
    sbs = sb_origins(w, h)
    out = {"desc": [], "best_sad": [], "best_mv": [], "inloop_mv": []}
    for l, ref in enumerate(refs):
        border = SUBPEL_BORDER if use_subpel else BORDER
        rp = pad_plane(ref, border)
        d = area(ctr[l], sbs, w, h, (w, 0, 0), (rp.shape[1], border, border), area_w, area_h)
        sad, mv = fullpel(src.reshape(-1), w, rp.reshape(-1), rp.shape[1], d)
        if use_subpel:
            sad, mv = subpel(src.reshape(-1), w, rp.reshape(-1), rp.shape[1], d, sad, mv, trace=trace)
        out["desc"].append(d), out["best_sad"].append(sad), out["best_mv"].append(mv), out["inloop_mv"].append(pack(mv))
    return {k: np.stack(v) for k, v in out.items()}


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def fixture_cases(fx):
    """[(name, src, refs, centers, area_w, area_h, expected dict)] of the fixture"""
    out = []
    for c, name in enumerate(fx["names"]):
        n_lists = int(fx[f"c{c}_lists"])
        exp = {k: fx[f"c{c}_{k}"] for k in ("desc", "best_sad", "best_mv", "inloop_mv", "sub_best_sad", "sub_best_mv", "sub_inloop_mv", "sub_stale")}
        out.append((str(name), fx[f"c{c}_src"], [fx[f"c{c}_ref{l}"] for l in range(n_lists)], fx[f"c{c}_centers"], int(fx[f"c{c}_area"][0]),
                    int(fx[f"c{c}_area"][1]), exp))
    return out


# ------------------------------------------------------------------------------------------------ sub-pel refinement (use_subpel_flag = 1)

SUBPEL_BORDER = 68   # the interpolated planes reach 3 samples before the window and 4 beyond its last block: 66 / 67 samples beyond the picture
# candidate order of both refinements: L, R, T, B, TL, TR, BR, BL (:4145-4161, :5045-5061)
CAND_DX = (-1, 1, 0, 0, -1, 1, 1, -1)
CAND_DY = (0, 0, -1, 1, -1, -1, 1, 1)
# psub_pel_direction: the first match of :4272-4295 walks L, R, T, B, TL, TR, BL, BR
LEFT, RIGHT, TOP, BOTTOM, TOP_LEFT, TOP_RIGHT, BOTTOM_LEFT, BOTTOM_RIGHT = range(8)
DIRECTION_WALK = ((0, LEFT), (1, RIGHT), (2, TOP), (3, BOTTOM), (4, TOP_LEFT), (5, TOP_RIGHT), (7, BOTTOM_LEFT), (6, BOTTOM_RIGHT))
# the three directions that keep a quarter-pel candidate valid when the half-pel vector is on the full-pel / half-pel grid (:5035-5042),
# candidate order; with a half-pel phase set the opposite directions count (:5023-5030)
VALID_FULL = ((BOTTOM_LEFT, LEFT, TOP_LEFT), (TOP_RIGHT, RIGHT, BOTTOM_RIGHT), (TOP_LEFT, TOP, TOP_RIGHT), (BOTTOM_RIGHT, BOTTOM, BOTTOM_LEFT),
              (LEFT, TOP_LEFT, TOP), (TOP, TOP_RIGHT, RIGHT), (RIGHT, BOTTOM_RIGHT, BOTTOM), (BOTTOM, BOTTOM_LEFT, LEFT))
OPPOSITE = {LEFT: RIGHT, RIGHT: LEFT, TOP: BOTTOM, BOTTOM: TOP, TOP_LEFT: BOTTOM_RIGHT, BOTTOM_RIGHT: TOP_LEFT, TOP_RIGHT: BOTTOM_LEFT,
            BOTTOM_LEFT: TOP_RIGHT}
# the buffer pairs of set_quarterpel_refinement_inputs_on_the_fly_block (:5229-5314): per method and candidate (plane, dx, dy) twice;
# planes 0 = A (full), 1 = b, 2 = h, 3 = j
QUARTER_PAIRS = (
    (((1, 0, 0), (0, 0, 0)), ((0, 0, 0), (1, 1, 0)), ((2, 0, 0), (0, 0, 0)), ((0, 0, 0), (2, 0, 1)), ((1, 0, 0), (2, 0, 0)), ((2, 0, 0), (1, 1, 0)),
     ((2, 0, 1), (1, 1, 0)), ((1, 0, 0), (2, 0, 1))),
    (((0, -1, 0), (1, 0, 0)), ((1, 0, 0), (0, 0, 0)), ((3, 0, 0), (1, 0, 0)), ((1, 0, 0), (3, 0, 1)), ((2, -1, 0), (1, 0, 0)), ((1, 0, 0), (2, 0, 0)),
     ((1, 0, 0), (2, 0, 1)), ((2, -1, 1), (1, 0, 0))),
    (((3, 0, 0), (2, 0, 0)), ((2, 0, 0), (3, 1, 0)), ((0, 0, -1), (2, 0, 0)), ((2, 0, 0), (0, 0, 0)), ((1, 0, -1), (2, 0, 0)), ((2, 0, 0), (1, 1, -1)),
     ((2, 0, 0), (1, 1, 0)), ((1, 0, 0), (2, 0, 0))),
    (((2, -1, 0), (3, 0, 0)), ((3, 0, 0), (2, 0, 0)), ((1, 0, -1), (3, 0, 0)), ((3, 0, 0), (1, 0, 0)), ((2, -1, 0), (1, 0, -1)), ((1, 0, -1), (2, 0, 0)),
     ((1, 0, 0), (2, 0, 0)), ((2, -1, 0), (1, 0, 0))))
# neither refinement walks these four shapes (:4330-4984, :5354-5990 have no loop for them): their 136 blocks keep the full-pel result
NOT_REFINED = {(4, 16), (16, 4), (64, 16), (16, 64)}
PLANE_MARGIN = 2   # the restatement's planes start this many samples before the window and end 4 beyond its last block: what the walks can reach


def _f4(a, b, c, d):
    return np.clip((-2 * a + 18 * b + 18 * c - 2 * d + 16) >> 5, 0, 255)


def interpolate(ref_plane, ref_stride, d):
    """the window and its three half-pel planes as int32 arrays indexed [y + PLANE_MARGIN][x + PLANE_MARGIN] in search coordinates:
    b[x] between x - 1 and x, h[y] between y - 1 and y, j the vertical filter of the rounded b (:4007-4094)"""
    ro, sw, sh = int(d[1]), int(d[4]), int(d[5])
    m = PLANE_MARGIN
    rows, cols = sh + 63 + m + 4, sw + 63 + m + 4
    a = np.lib.stride_tricks.as_strided(ref_plane[ro - m * ref_stride - m:], (rows, cols), (ref_stride, 1)).astype(np.int32)
    b, h, j = np.zeros_like(a), np.zeros_like(a), np.zeros_like(a)
    b[:, 2:-1] = _f4(a[:, :-3], a[:, 1:-2], a[:, 2:-1], a[:, 3:])
    h[2:-1, :] = _f4(a[:-3, :], a[1:-2, :], a[2:-1, :], a[3:, :])
    j[2:-1, :] = _f4(b[:-3, :], b[1:-2, :], b[2:-1, :], b[3:, :])
    return a, b, h, j


def _cost(src_blk, plane_blk):
    """twice the SAD over every second row (USE_INLOOP_ME_FULL_SAD 0)"""
    return 2 * int(np.abs(src_blk[::2] - plane_blk[::2]).sum())


def subpel_sb(src_plane, src_stride, ref_plane, ref_stride, d, best_sad, best_mv, side_4_only=False, trace=None):
    """refines one superblock's [849] arrays in place: half-pel (:4304-4984) then quarter-pel (:5320-5990).  The walk is over the raster
    candidates of every shape the reference walks (NOT_REFINED keep their full-pel result); candidate c refines buffer slot PACK_SOURCE[c]
    on the samples of the block at c's raster place."""
    so, ro, xo, yo, sw, sh, bw, bh = (int(v) for v in d)
    src = np.zeros((64, 64), np.int32)
    src[:bh, :bw] = np.lib.stride_tricks.as_strided(src_plane[so:], (bh, bw), (src_stride, 1))
    planes = interpolate(ref_plane, ref_stride, d)
    m = PLANE_MARGIN
    i16 = lambda v: ((int(v) & 0xFFFF) ^ 0x8000) - 0x8000  # noqa: E731
    word = lambda x, y: ((y & 0xFFFF) << 16) | (x & 0xFFFF)  # noqa: E731
    direction = np.zeros(N_BLOCKS, np.int32)
    geometry = []
    for w, h, start in SHAPES:
        if (w, h) in NOT_REFINED:
            continue
        cols = 64 // w
        for r in range(cols * (64 // h)):
            geometry.append((start + r, (r % cols) * w, (r // cols) * h, w, h))
    for stage in (0, 1):
        for c, bx, by, w, h in geometry:
            slot = int(PACK_SOURCE[c])
            if side_4_only and not SIDE_4[slot]:
                continue
            if stage == 1 and (w, h) == (32, 32):
                by >>= 5    # the quarter-pel walk of the 32x32 blocks forms block_shift_y without its << 5 (:5965): the two lower blocks are
                            # measured on the source and reference samples one row below the upper ones
            s = src[by:by + h, bx:bx + w]
            x_mv, y_mv = i16(best_mv[slot] & 0xFFFF), i16(best_mv[slot] >> 16)
            blk = lambda p, x, y: planes[p][m + y + by:m + y + by + h, m + x + bx:m + x + bx + w]  # noqa: E731
            if stage == 0:
                xs, ys = (x_mv >> 2) - xo, (y_mv >> 2) - yo
                where = ((1, 0, 0), (1, 1, 0), (2, 0, 0), (2, 0, 1), (3, 0, 0), (3, 1, 0), (3, 1, 1), (3, 0, 1))
                dist = []
                for k, (p, dx, dy) in enumerate(where):
                    dist.append(_cost(s, blk(p, xs + dx, ys + dy)))
                    if dist[k] < best_sad[slot]:
                        best_sad[slot], best_mv[slot] = dist[k], word(x_mv + 2 * CAND_DX[k], y_mv + 2 * CAND_DY[k])
                lo = min(dist)
                direction[slot] = next(name for k, name in DIRECTION_WALK if dist[k] == lo)
            else:
                xs, ys = ((x_mv + 2) >> 2) - xo, ((y_mv + 2) >> 2) - yo
                method = (y_mv & 2) + ((x_mv & 2) >> 1)
                if trace is not None:
                    trace.append((method, int(direction[slot])))
                for k in range(8):
                    valid = VALID_FULL[k] if method == 0 else tuple(OPPOSITE[v] for v in VALID_FULL[k])
                    if direction[slot] not in valid:
                        continue
                    (p1, dx1, dy1), (p2, dx2, dy2) = QUARTER_PAIRS[method][k]
                    dist = _cost(s, (blk(p1, xs + dx1, ys + dy1) + blk(p2, xs + dx2, ys + dy2) + 1) >> 1)
                    if dist < best_sad[slot]:
                        best_sad[slot], best_mv[slot] = dist, word(x_mv + CAND_DX[k], y_mv + CAND_DY[k])


def subpel(src_plane, src_stride, ref_plane, ref_stride, desc, best_sad, best_mv, side_4_only=False, trace=None):
    sad, mv = best_sad.astype(np.int64), best_mv.astype(np.int64)
    for i, d in enumerate(desc):
        subpel_sb(src_plane, src_stride, ref_plane, ref_stride, d, sad[i], mv[i], side_4_only, trace)
    return sad.astype(np.uint32), mv.astype(np.uint32)
