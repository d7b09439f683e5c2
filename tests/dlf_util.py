"""CPU restatement of the reference's AV1 deblocking filter and of its filter-level search (Source/Lib/Codec/EbDeblockingFilter.c), for the
tests of the device entries.  TEST INFRASTRUCTURE: numpy only, no reference code.

  sample filters   filter4/6/8/14 and their masks (:51-396, highbd :398-712) once, on arrays of lines, in the 16-bit form: at bd == 8 its
                   shifts vanish and it is the 8-bit form.
  decisions        set_lpf_parameters (:1004-1123) on the svthip_lf_mi grid (LF_MI_DTYPE, one cell per 4x4 luma samples).
  frame filter     two forms.  loop_filter_frame(..., literal=True) keeps the reference's order: superblock by superblock, the vertical
                   edges of SB c, then the horizontal edges of SB c - 1, each with the walk that advances by the transform size of the
                   cell it stands on.  literal=False is two whole-plane passes, every edge of a pass at once per filter length.  That the
                   two agree is what the device kernels rest on (tests/test_dlf_vs_ref.py).
  search           plane_sse, sse_table (try_filter_frame :1773-1827 for every level), level_walk (search_filter_level :1828-1989 over
                   a table, with the set of levels it asked for) and pick_filter_level (the LPF_PICK_FROM_FULL_IMAGE arm, :2065-2091).

Planes are 2-D arrays of the plane's size (luma w x h, chroma w/2 x h/2); levels = (luma vertical, luma horizontal, Cb, Cr).
"""
import numpy as np

from abi_util import svtav1_hip

LF_MI_DTYPE = svtav1_hip.LF_MI_DTYPE   # read from include/svtav1_hip.h by the package

# BlockSize and TxSize in the reference's enum order (Codec/EbDefinitions.h)
BLOCK_W = np.array([4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64])
BLOCK_H = np.array([4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16])
TX_W = np.array([4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64])
TX_H = np.array([4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16])
BLOCK_OF = {(int(w), int(h)): i for i, (w, h) in enumerate(zip(BLOCK_W, BLOCK_H))}
TX_OF = {(int(w), int(h)): i for i, (w, h) in enumerate(zip(TX_W, TX_H))}
MAX_LOOP_FILTER = 63


def new_stats():
    """what the sample filters and decisions met; filled when passed down"""
    return {"len": set(), "mask_fail": set(), "hev": set(), "no_hev": set(), "flat": set(), "no_flat": set(), "flat2": set(), "no_flat2": set(),
            "clamp_lo": 0, "clamp_hi": 0, "skip_both_pu": 0, "skip_both_inner": 0, "skip_one": 0, "sb_edge": set(), "partial_sb_edge": set()}


# ---------------------------------------------------------------- limits

def limits(level, sharpness):
    """(mblim, lim, hev_thr) of update_sharpness (:719-738) and av1_loop_filter_init (:802-803)"""
    inside = level >> ((sharpness > 0) + (sharpness > 4))
    if sharpness > 0 and inside > 9 - sharpness:
        inside = 9 - sharpness
    inside = max(inside, 1)
    return 2 * (level + 2) + inside, inside, level >> 4


# ---------------------------------------------------------------- sample filters on [n] lines

def _clamp(t, bd, st, live):
    """signed_char_clamp; saturations are counted only on the lines in `live`, whose result is written"""
    lo = -(128 << (bd - 8))
    if st is not None:
        st["clamp_lo"] += int(np.count_nonzero((t < lo) & live))
        st["clamp_hi"] += int(np.count_nonzero((t > -lo - 1) & live))
    return np.clip(t, lo, -lo - 1)


def _filter4(p1, p0, q0, q1, mask, thresh, bd, st, key, live):
    sh = bd - 8
    off = 0x80 << sh
    ps1, ps0, qs0, qs1 = p1 - off, p0 - off, q0 - off, q1 - off
    hev = (np.abs(p1 - p0) > (thresh << sh)) | (np.abs(q1 - q0) > (thresh << sh))
    if st is not None:
        if np.any(hev & mask):
            st["hev"].add(key)
        if np.any(~hev & mask):
            st["no_hev"].add(key)
    f = np.where(hev, _clamp(ps1 - qs1, bd, st, live & hev), 0)
    f = np.where(mask, _clamp(f + 3 * (qs0 - ps0), bd, st, live), 0)
    f1 = _clamp(f + 4, bd, st, live) >> 3
    f2 = _clamp(f + 3, bd, st, live) >> 3
    oq0 = _clamp(qs0 - f1, bd, st, live) + off
    op0 = _clamp(ps0 + f2, bd, st, live) + off
    f = np.where(hev, 0, (f1 + 1) >> 1)
    oq1 = _clamp(qs1 - f, bd, st, live) + off
    op1 = _clamp(ps1 + f, bd, st, live) + off
    return op1, op0, oq0, oq1


def _r(v, n):
    return (v + (1 << (n - 1))) >> n


def filter_lines(t, length, level, sharpness, bd, st=None, key=None):
    """t: int32 [n][2K] taps p(K-1) .. p0 q0 .. q(K-1) across the edge (K = 2, 3, 4, 7 for length 4, 6, 8, 14); returns the filtered taps"""
    mblim, lim, thr = limits(level, sharpness)
    sh = bd - 8
    lim16, blim16, one = lim << sh, mblim << sh, 1 << sh
    K = t.shape[1] // 2
    p = [t[:, K - 1 - i] for i in range(K)]
    q = [t[:, K + i] for i in range(K)]
    d = np.abs
    mask = (d(p[1] - p[0]) <= lim16) & (d(q[1] - q[0]) <= lim16) & (d(p[0] - q[0]) * 2 + d(p[1] - q[1]) // 2 <= blim16)
    if length >= 6:
        mask &= (d(p[2] - p[1]) <= lim16) & (d(q[2] - q[1]) <= lim16)
    if length >= 8:
        mask &= (d(p[3] - p[2]) <= lim16) & (d(q[3] - q[2]) <= lim16)
    if st is not None:
        st["len"].add(key)
        if not np.all(mask):
            st["mask_fail"].add(key)
    if length == 4:
        flat = np.zeros_like(mask)
    else:
        flat = (d(p[1] - p[0]) <= one) & (d(q[1] - q[0]) <= one) & (d(p[2] - p[0]) <= one) & (d(q[2] - q[0]) <= one) & mask
        if length >= 8:
            flat &= (d(p[3] - p[0]) <= one) & (d(q[3] - q[0]) <= one)
    o = t.copy()
    op1, op0, oq0, oq1 = _filter4(p[1], p[0], q[0], q[1], mask, thr, bd, st, key, mask & ~flat)   # flat lines overwrite filter4's result
    o[:, K - 2], o[:, K - 1], o[:, K], o[:, K + 1] = op1, op0, oq0, oq1
    if length == 4:
        return o
    if length == 6:
        new = {K - 2: _r(p[2] * 3 + p[1] * 2 + p[0] * 2 + q[0], 3), K - 1: _r(p[2] + p[1] * 2 + p[0] * 2 + q[0] * 2 + q[1], 3),
               K: _r(p[1] + p[0] * 2 + q[0] * 2 + q[1] * 2 + q[2], 3), K + 1: _r(p[0] + q[0] * 2 + q[1] * 2 + q[2] * 3, 3)}
    else:
        new = {K - 3: _r(p[3] * 3 + 2 * p[2] + p[1] + p[0] + q[0], 3), K - 2: _r(p[3] * 2 + p[2] + 2 * p[1] + p[0] + q[0] + q[1], 3),
               K - 1: _r(p[3] + p[2] + p[1] + 2 * p[0] + q[0] + q[1] + q[2], 3), K: _r(p[2] + p[1] + p[0] + 2 * q[0] + q[1] + q[2] + q[3], 3),
               K + 1: _r(p[1] + p[0] + q[0] + 2 * q[1] + q[2] + q[3] * 2, 3), K + 2: _r(p[0] + q[0] + q[1] + 2 * q[2] + q[3] * 3, 3)}
    if st is not None:
        st["flat" if np.any(flat) else "no_flat"].add(key)
        if np.any(flat) and np.any(~flat & mask):
            st["no_flat"].add(key)
    for c, v in new.items():
        o[:, c] = np.where(flat, v, o[:, c])
    if length == 14:
        flat2 = (d(p[4] - p[0]) <= one) & (d(q[4] - q[0]) <= one) & (d(p[5] - p[0]) <= one) & (d(q[5] - q[0]) <= one) & \
            (d(p[6] - p[0]) <= one) & (d(q[6] - q[0]) <= one) & flat
        if st is not None:
            if np.any(flat2):
                st["flat2"].add(key)
            if np.any(flat & ~flat2):
                st["no_flat2"].add(key)
        P, Q = p, q
        wide = {K - 6: P[6] * 7 + P[5] * 2 + P[4] * 2 + P[3] + P[2] + P[1] + P[0] + Q[0],
                K - 5: P[6] * 5 + P[5] * 2 + P[4] * 2 + P[3] * 2 + P[2] + P[1] + P[0] + Q[0] + Q[1],
                K - 4: P[6] * 4 + P[5] + P[4] * 2 + P[3] * 2 + P[2] * 2 + P[1] + P[0] + Q[0] + Q[1] + Q[2],
                K - 3: P[6] * 3 + P[5] + P[4] + P[3] * 2 + P[2] * 2 + P[1] * 2 + P[0] + Q[0] + Q[1] + Q[2] + Q[3],
                K - 2: P[6] * 2 + P[5] + P[4] + P[3] + P[2] * 2 + P[1] * 2 + P[0] * 2 + Q[0] + Q[1] + Q[2] + Q[3] + Q[4],
                K - 1: P[6] + P[5] + P[4] + P[3] + P[2] + P[1] * 2 + P[0] * 2 + Q[0] * 2 + Q[1] + Q[2] + Q[3] + Q[4] + Q[5],
                K: P[5] + P[4] + P[3] + P[2] + P[1] + P[0] * 2 + Q[0] * 2 + Q[1] * 2 + Q[2] + Q[3] + Q[4] + Q[5] + Q[6],
                K + 1: P[4] + P[3] + P[2] + P[1] + P[0] + Q[0] * 2 + Q[1] * 2 + Q[2] * 2 + Q[3] + Q[4] + Q[5] + Q[6] * 2,
                K + 2: P[3] + P[2] + P[1] + P[0] + Q[0] + Q[1] * 2 + Q[2] * 2 + Q[3] * 2 + Q[4] + Q[5] + Q[6] * 3,
                K + 3: P[2] + P[1] + P[0] + Q[0] + Q[1] + Q[2] * 2 + Q[3] * 2 + Q[4] * 2 + Q[5] + Q[6] * 4,
                K + 4: P[1] + P[0] + Q[0] + Q[1] + Q[2] + Q[3] * 2 + Q[4] * 2 + Q[5] * 2 + Q[6] * 5,
                K + 5: P[0] + Q[0] + Q[1] + Q[2] + Q[3] + Q[4] * 2 + Q[5] * 2 + Q[6] * 7}
        for c, v in wide.items():
            o[:, c] = np.where(flat2, _r(v, 4), o[:, c])
    return o


_TAPS = {4: 2, 6: 3, 8: 4, 14: 7}


def apply_edges(img, uy, ux, length, direction, level, sharpness, bd, st=None, plane=0):
    """filters, in place, the 4-sample edges of `length` that start at the 4x4 units (uy, ux): vertical edges (direction 0) at x = 4 ux over
    rows 4 uy .. + 3, horizontal edges at y = 4 uy over columns 4 ux .. + 3"""
    if len(uy) == 0:
        return
    K = _TAPS[length]
    line = (4 * (uy if direction == 0 else ux)[:, None] + np.arange(4)[None, :]).reshape(-1)
    across = (4 * np.repeat(ux if direction == 0 else uy, 4))[:, None] + np.arange(-K, K)[None, :]
    rows, cols = (line[:, None], across) if direction == 0 else (across, line[:, None])
    t = img[rows, cols].astype(np.int32)
    img[rows, cols] = filter_lines(t, length, level, sharpness, bd, st, (plane, direction, length)).astype(img.dtype)


# ---------------------------------------------------------------- decisions

def plane_geometry(mi, plane):
    """per 4x4 unit of the plane: transform width and height, prediction block width and height (in samples of the plane) and the skip flag
    of the cell set_lpf_parameters reads (chroma: the odd cell)"""
    c = mi if plane == 0 else mi[1::2, 1::2]
    sb = c["sb_type"].astype(np.int64)
    if plane == 0:
        tx = c["tx_size"].astype(np.int64)
        return TX_W[tx], TX_H[tx], BLOCK_W[sb], BLOCK_H[sb], (c["flags"] & 1).astype(bool)
    pw, ph = np.maximum(BLOCK_W[sb] // 2, 4), np.maximum(BLOCK_H[sb] // 2, 4)   # ss_size_lookup[..][1][1]
    return np.minimum(pw, 32), np.minimum(ph, 32), pw, ph, (c["flags"] & 1).astype(bool)   # av1_get_max_uv_txsize


def edge_lengths(mi, plane, direction, pw, ph, level, st=None):
    """[ph / 4][pw / 4] filter length (0, 4, 6, 8, 14) of the edge that starts each unit, for a plane of pw x ph samples"""
    txw, txh, bw, bh, skip = plane_geometry(mi, plane)
    nuy, nux = ph // 4, pw // 4
    tx, bl = (txw, bw) if direction == 0 else (txh, bh)
    tx, bl, skip = tx[:nuy, :nux], bl[:nuy, :nux], skip[:nuy, :nux]
    coord = 4 * (np.arange(nux)[None, :] if direction == 0 else np.arange(nuy)[:, None]) + np.zeros((nuy, nux), np.int64)
    pv_tx, pv_skip = np.roll(tx, 1, axis=1 - direction), np.roll(skip, 1, axis=1 - direction)
    edge = ((coord & (tx - 1)) == 0) & (coord > 0)
    pu_edge = (coord & (bl - 1)) == 0
    on = edge & (level != 0) & (~pv_skip | ~skip | pu_edge)
    m = np.minimum(tx, pv_tx)
    length = np.where(m == 4, 4, np.where(m == 8, 8 if plane == 0 else 6, 14 if plane == 0 else 6))
    if st is not None and level != 0:
        st["skip_both_pu"] += int(np.count_nonzero(edge & pv_skip & skip & pu_edge))
        st["skip_both_inner"] += int(np.count_nonzero(edge & pv_skip & skip & ~pu_edge))
        st["skip_one"] += int(np.count_nonzero(edge & (pv_skip ^ skip)))
        full = (pw if direction == 0 else ph) // (64 >> (plane > 0)) * (64 >> (plane > 0))
        if np.any(on & (coord % (64 >> (plane > 0)) == 0)):
            st["sb_edge"].add((plane, direction))
        if np.any(on & (coord == full)):
            st["partial_sb_edge"].add((plane, direction))
    return np.where(on, length, 0)


def set_lpf_parameters(mi, plane, direction, x, y, pw, ph, level):
    """(filter length, transform dimension in the direction) at plane position (x, y): the scalar form the literal walk uses"""
    if x >= pw or y >= ph:
        return 0, 4
    ss = int(plane > 0)
    r, c = ss | ((y << ss) >> 2), ss | ((x << ss) >> 2)

    def dims(cell):
        sb = int(cell["sb_type"])
        if plane == 0:
            return (int(TX_W[cell["tx_size"]]), int(TX_H[cell["tx_size"]]))[direction], (int(BLOCK_W[sb]), int(BLOCK_H[sb]))[direction]
        p = max(int((BLOCK_W, BLOCK_H)[direction][sb]) // 2, 4)
        return min(p, 32), p

    cur = mi[r, c]
    ts, bl = dims(cur)
    coord = x if direction == 0 else y
    if coord & (ts - 1) or coord == 0:
        return 0, ts
    prev = mi[r, c - (1 << ss)] if direction == 0 else mi[r - (1 << ss), c]
    pv_ts, _ = dims(prev)
    pu_edge = not (coord & (bl - 1))
    if level and (not (prev["flags"] & 1) or not (cur["flags"] & 1) or pu_edge):
        m = min(ts, pv_ts)
        return (4 if m == 4 else (8 if plane == 0 else 6) if m == 8 else (14 if plane == 0 else 6)), ts
    return 0, ts


# ---------------------------------------------------------------- frame filter

def _plane_levels(levels, plane):
    return (levels[0], levels[1]) if plane == 0 else (levels[1 + plane], levels[1 + plane])


def filter_plane_passes(img, mi, plane, lv, sharpness, bd, st=None, passes=(0, 1)):
    """form (b): one whole-plane pass per direction"""
    ph, pw = img.shape
    for direction in passes:
        L = edge_lengths(mi, plane, direction, pw, ph, lv[direction], st)
        for length in (4, 6, 8, 14):
            uy, ux = np.nonzero(L == length)
            apply_edges(img, uy, ux, length, direction, lv[direction], sharpness, bd, st, plane)


def _filter_block_plane(img, mi, plane, direction, sb_r, sb_c, lv, sharpness, bd):
    """av1_filter_block_plane_vert / _horz (:1125-1380) of one 64x64 superblock"""
    ph, pw = img.shape
    n = 16 >> (plane > 0)
    x0, y0 = (sb_c * 64) >> (plane > 0), (sb_r * 64) >> (plane > 0)
    for a in range(n):
        b = 0
        while b < n:
            x, y = (x0 + 4 * b, y0 + 4 * a) if direction == 0 else (x0 + 4 * a, y0 + 4 * b)
            length, ts = set_lpf_parameters(mi, plane, direction, x, y, pw, ph, lv[direction])
            if length:
                apply_edges(img, np.array([y // 4]), np.array([x // 4]), length, direction, lv[direction], sharpness, bd, None, plane)
            b += ts // 4


def loop_filter_frame(planes, mi, levels, sharpness, plane_start, plane_end, bd, literal=False, st=None):
    """av1_loop_filter_frame (:1462-1501): filters planes[plane_start : plane_end] in place"""
    h, w = planes[0].shape
    sb_rows, sb_cols = (h + 63) // 64, (w + 63) // 64
    for plane in range(plane_start, plane_end):
        if plane == 0 and not levels[0] and not levels[1]:
            break       # the reference leaves the loop here (:1409-1410): the chroma planes after it stay as they are
        if plane > 0 and not levels[1 + plane]:
            continue
        lv = _plane_levels(levels, plane)
        if not literal:
            filter_plane_passes(planes[plane], mi, plane, lv, sharpness, bd, st)
            continue
        for r in range(sb_rows):
            for c in range(sb_cols):
                _filter_block_plane(planes[plane], mi, plane, 0, r, c, lv, sharpness, bd)
                if c > 0:
                    _filter_block_plane(planes[plane], mi, plane, 1, r, c - 1, lv, sharpness, bd)
                if c == sb_cols - 1:
                    _filter_block_plane(planes[plane], mi, plane, 1, r, c, lv, sharpness, bd)


# ---------------------------------------------------------------- search

def plane_sse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int(np.sum(d * d))


def try_levels(levels, plane, direction, level):
    """the four levels try_filter_frame filters `plane` with for candidate `level` (:1787-1815)"""
    lv = list(levels)
    if plane == 0:
        if direction in (0, 2):
            lv[0] = level
        if direction in (1, 2):
            lv[1] = level
    else:
        lv[1 + plane] = level
    return lv


def sse_table(recon, source, mi, plane, direction, levels, sharpness, bd, only=range(64)):
    """{level: what try_filter_frame(level, plane, direction) returns}"""
    out = {}
    for level in only:
        img = recon[plane].copy()
        lv = _plane_levels(try_levels(levels, plane, direction, level), plane)
        filter_plane_passes(img, mi, plane, lv, sharpness, bd)
        out[level] = plane_sse(img, source[plane])
    return out


def level_walk(table, start_level, only_4x4, st=None):
    """(level, visited mask, levels in the order asked) of search_filter_level's walk (:1852-1985); table[level] is asked only for the
    levels the reference tries"""
    mask = 0
    ss = {}
    order = []

    def err(level):
        nonlocal mask
        if level not in ss:
            mask |= 1 << level
            order.append(level)
            ss[level] = int(table[level])
        return ss[level]

    mid = min(max(int(start_level), 0), MAX_LOOP_FILTER)
    step = 4 if mid < 16 else mid // 4
    direction = 0
    if st is not None:
        st["start_low" if mid < 16 else "start_high"] = True
    best_err = err(mid)
    best = mid
    while step > 0:
        high, low = min(mid + step, MAX_LOOP_FILTER), max(mid - step, 0)
        bias = (best_err >> (15 - mid // 8)) * step
        if not only_4x4:
            bias >>= 1
        if st is not None:
            st["clamp0"] |= mid - step < 0
            st["clamp63"] |= mid + step > MAX_LOOP_FILTER
        if direction <= 0 and low != mid:
            e = err(low)
            if e < best_err + bias:
                if e < best_err:
                    best_err = e
                elif st is not None:
                    st["low_near_tie"] = True
                best = low
        if direction >= 0 and high != mid:
            e = err(high)
            if e < best_err - bias:
                best_err = e
                best = high
            elif st is not None and e < best_err:
                st["high_within_bias"] = True
        if best == mid:
            step //= 2
            direction = 0
            if st is not None:
                st["halved"] = True
        else:
            direction = -1 if best < mid else 1
            mid = best
    return best, mask, order


def new_walk_stats():
    return {k: False for k in ("start_low", "start_high", "clamp0", "clamp63", "halved", "low_near_tie", "high_within_bias")}


class _LazyTable:
    def __init__(self, fn):
        self.fn, self.got = fn, {}

    def __getitem__(self, level):
        if level not in self.got:
            self.got[level] = self.fn(level)
        return self.got[level]


# the five searches of av1_pick_filter_level (:2072-2089): plane, direction, index of the start level in last_frame_filter_level (the tied
# search reads last_frame_filter_level[dir] with dir == 2, :1847), and the levels its result is stored to
PICK_RUNS = ((0, 2, 2, (0, 1)), (0, 0, 0, (0,)), (0, 1, 1, (1,)), (1, 0, 2, (2,)), (2, 0, 3, (3,)))


def pick_filter_level(recon, source, mi, last_levels, sharpness, only_4x4, bd, tables=None, st=None):
    """(levels[4], [visited mask of each of the five walks], trace); with `tables` (five full tables) nothing is filtered.  trace: the
    four levels of every frame filtering the reference would run, in its order"""
    levels = [int(v) for v in last_levels]
    masks, trace = [], []
    for i, (plane, direction, start, store) in enumerate(PICK_RUNS):
        if tables is not None:
            t = tables[i]
        else:
            cur = list(levels)
            t = _LazyTable(lambda level, cur=cur, plane=plane, direction=direction:
                           sse_table(recon, source, mi, plane, direction, cur, sharpness, bd, only=(level,))[level])
        best, mask, order = level_walk(t, last_levels[start], only_4x4, st)
        trace += [try_levels(levels, plane, direction, level) for level in order]
        for k in store:
            levels[k] = best
        masks.append(mask)
    return levels, masks, trace


# ---------------------------------------------------------------- test pictures

def random_mi_grid(rng, w, h, p_skip=0.3, min_size=4):
    """a valid partition of every 64x64 superblock into the 22 block sizes, each block with one transform size that tiles it"""
    rows, cols = (h + 63) // 64 * 16, (w + 63) // 64 * 16
    mi = np.zeros((rows, cols), LF_MI_DTYPE)

    def leaf(x, y, bw, bh):
        options = [(tw, th) for (tw, th) in TX_OF if tw <= bw and th <= bh and bw % tw == 0 and bh % th == 0]
        biggest = max(options, key=lambda t: t[0] * t[1])
        tw, th = biggest if rng.random() < 0.6 else options[rng.integers(len(options))]
        cell = mi[y // 4:(y + bh) // 4, x // 4:(x + bw) // 4]
        cell["sb_type"], cell["tx_size"], cell["flags"] = BLOCK_OF[(bw, bh)], TX_OF[(tw, th)], int(rng.random() < p_skip)

    def node(x, y, s):
        k = rng.integers(10)
        if s > 8 and (k < 4 or (s == 64 and k < 5)):
            for dy in (0, s // 2):
                for dx in (0, s // 2):
                    node(x + dx, y + dy, s // 2)
        elif k == 6 and s // 2 >= min_size:
            leaf(x, y, s, s // 2), leaf(x, y + s // 2, s, s // 2)
        elif k == 7 and s // 2 >= min_size:
            leaf(x, y, s // 2, s), leaf(x + s // 2, y, s // 2, s)
        elif k == 8 and s >= 16 and s // 4 >= min_size:
            for i in range(4):
                leaf(x, y + i * s // 4, s, s // 4)
        elif k == 9 and s >= 16 and s // 4 >= min_size:
            for i in range(4):
                leaf(x + i * s // 4, y, s // 4, s)
        elif s == 8 and k < 3 and min_size <= 4:
            for dy in (0, 4):
                for dx in (0, 4):
                    leaf(x + dx, y + dy, 4, 4)
        else:
            leaf(x, y, s, s)

    for y in range(0, rows * 4, 64):
        for x in range(0, cols * 4, 64):
            node(x, y, 64)
    return mi


def random_picture(rng, w, h, bd, mi):
    """(recon planes, source planes): a smooth source; the reconstruction is the source plus an offset per transform block and noise, both
    of a strength drawn per 32x32 area, so that flat runs, ordinary edges and saturating steps all occur"""
    mx = (1 << bd) - 1
    sc = 1 << (bd - 8)
    recon, source = [], []
    for plane in range(3):
        pw, ph = (w, h) if plane == 0 else (w // 2, h // 2)
        yy, xx = np.mgrid[0:ph, 0:pw]
        base = (128 + 60 * np.sin(xx / 37.0 + plane) + 50 * np.cos(yy / 29.0)) * sc
        txw, txh, _, _, _ = plane_geometry(mi, plane)
        uy, ux = yy // 4, xx // 4
        bx, by = xx // np.maximum(txw[uy, ux], 4), yy // np.maximum(txh[uy, ux], 4)
        area = (yy // 32) * 64 + xx // 32
        amp = np.array([0, 1, 1, 3, 12, 60, 250])[rng.integers(0, 7, 4096)][area] * sc
        noise = np.array([0, 0, 1, 2, 6, 120])[rng.integers(0, 6, 4096)][area] * sc
        off = rng.integers(-1000, 1001, (ph // 4 + 1, pw // 4 + 1))[by % (ph // 4 + 1), bx % (pw // 4 + 1)] / 1000.0
        rec = base + off * amp + rng.integers(-1000, 1001, (ph, pw)) / 1000.0 * noise
        flatten = (np.array(rng.integers(0, 3, 4096) == 0)[area])
        rec = np.where(flatten, np.round(base / (16 * sc)) * 16 * sc + np.round(off * amp), rec)
        src = base + rng.integers(-2 * sc, 2 * sc + 1, (ph, pw))
        dt = np.uint8 if bd == 8 else np.uint16
        recon.append(np.clip(np.round(rec), 0, mx).astype(dt))
        source.append(np.clip(np.round(src), 0, mx).astype(dt))
    return recon, source
