"""numpy / Python restatement of the reference's CDEF (Codec/EbCdef.c, EbCdefProcess.c), written from its C forms: the block lists
(sb_all_skip, sb_compute_cdef_list), cdef_find_dir_c, constrain, adjust_strength, cdef_filter_block_c / cdef_filter_fb, dist_8x8_16bit_c,
mse_4x4_16bit_c, compute_cdef_dist, cdef_seg_search[16bit], search_one_dual_c, joint_strength_search_dual, finish_cdef_search and
av1_cdef_frame[16bit].  CDEF_M = 1, fast = 0, 4:2:0, 64x64 superblocks, three planes, one tile.

The filter is written over whole planes at once: the picture sits in an array with a border of CDEF_VERY_LARGE, which is what every
filter block of the reference sees (its own tile from the deblocked picture, CDEF_VERY_LARGE outside the picture; av1_cdef_frame's line
and column buffers exist so that its in-place filter still reads pre-CDEF samples).  Per-sample maps carry each 8x8 block's direction and
strength.  `stats` (new_stats()) counts the arms the issue lists while a search or a frame filter runs."""
import os

import numpy as np

from abi_util import svtav1_hip

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
VERY_LARGE = 30000
PAD = 3
DIRECTIONS = (((-1, 1), (-2, 2)), ((0, 1), (-1, 2)), ((0, 1), (0, 2)), ((0, 1), (1, 2)), ((1, 1), (2, 2)), ((1, 0), (2, 1)), ((1, 0), (2, 0)),
              ((1, 0), (2, -1)))   # cdef_directions[dir][k] as (rows, columns)
PRI_TAPS = np.array(((4, 2), (3, 3)), np.int64)
SEC_TAPS = (2, 1)
DIV_TABLE = (0, 840, 420, 280, 210, 168, 140, 120, 105)
MSB = np.array([0] + [int(v).bit_length() - 1 for v in range(1, 1024)], np.int64)
RESULT_DTYPE = svtav1_hip.CDEF_RESULT_DTYPE   # read from include/svtav1_hip.h by the package
STAT_KEYS = ("copy", "pri0_sec", "adj0", "taps0", "taps1") + tuple(f"dir{d}" for d in range(8)) + (
    "clamp_min", "clamp_max", "border_top", "border_left", "border_bottom", "border_right", "frame_zero_pair", "frame_empty_list", "frame_filtered")


def new_stats():
    return {k: 0 for k in STAT_KEYS}


def geometry(w, h):
    """nhfb, nvfb"""
    return ((w >> 2) + 15) // 16, ((h >> 2) + 15) // 16


def ac_quant(qindex, bd):
    """av1_ac_quant_Q3(qindex, 0, bd), from the quantiser rows the project pins (tests/golden/quant_tables.npz: dequant[1] of luma)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "quant_tables.npz"))
    return int(z[f"rows_bd{bd}_inter"][qindex, 0, 9])


def cdef_lambda(qindex, bd):
    q = ac_quant(qindex, bd) >> (bd - 8)
    return .12 * q * q / 256.


# ---------------------------------------------------------------- lists
def block_lists(skip, w, h):
    """skip: [h / 4][w / 4] bytes.  -> listed [h / 8][w / 8] bool (is_8x8_block_skip is false), counted [nvfb][nhfb] bool (sb_all_skip is false)"""
    s = np.asarray(skip)[:h >> 2, :w >> 2] != 0
    listed = ~(s[0::2, 0::2] & s[0::2, 1::2] & s[1::2, 0::2] & s[1::2, 1::2])
    nh, nv = geometry(w, h)
    counted = np.zeros((nv, nh), bool)
    for r in range(nv):
        for c in range(nh):
            counted[r, c] = not s[r * 16:(r + 1) * 16, c * 16:(c + 1) * 16].all()
    return listed, counted


def per_fb(blocks, nv, nh):
    """sums of a per-8x8-block array over the filter blocks"""
    out = np.zeros((nv, nh), blocks.dtype)
    for r in range(nv):
        for c in range(nh):
            out[r, c] = blocks[r * 8:(r + 1) * 8, c * 8:(c + 1) * 8].sum(dtype=blocks.dtype)
    return out


# ---------------------------------------------------------------- directions
def find_dirs(luma, shift):
    """cdef_find_dir_c on every 8x8 block of the plane -> dir, var [h / 8][w / 8]"""
    h, w = luma.shape
    b = (luma.astype(np.int64) >> shift).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128
    n = b.shape[:2]
    partial = np.zeros(n + (8, 15), np.int64)
    for i in range(8):
        for j in range(8):
            x = b[:, :, i, j]
            for d, k in ((0, i + j), (1, i + j // 2), (2, i), (3, 3 + i - j // 2), (4, 7 + i - j), (5, 3 - i // 2 + j), (6, j), (7, i // 2 + j)):
                partial[:, :, d, k] += x
    cost = np.zeros(n + (8,), np.int64)
    sq = partial * partial
    cost[..., 2] = sq[..., 2, :8].sum(-1) * DIV_TABLE[8]
    cost[..., 6] = sq[..., 6, :8].sum(-1) * DIV_TABLE[8]
    for d in (0, 4):
        for i in range(7):
            cost[..., d] += (sq[..., d, i] + sq[..., d, 14 - i]) * DIV_TABLE[i + 1]
        cost[..., d] += sq[..., d, 7] * DIV_TABLE[8]
    for d in (1, 3, 5, 7):
        cost[..., d] = sq[..., d, 3:8].sum(-1) * DIV_TABLE[8]
        for j in range(3):
            cost[..., d] += (sq[..., d, j] + sq[..., d, 10 - j]) * DIV_TABLE[2 * j + 2]
    best_dir = np.zeros(n, np.int64)
    best_cost = np.zeros(n, np.int64)
    for d in range(8):                       # strict >: the first of equal costs
        m = cost[..., d] > best_cost
        best_cost[m], best_dir[m] = cost[..., d][m], d
    opp = np.take_along_axis(cost, ((best_dir + 4) & 7)[..., None], -1)[..., 0]
    return best_dir, (best_cost - opp) >> 10


def adjust_strength(strength, var):
    var = np.asarray(var, np.int64)
    v6 = var >> 6
    msb = np.floor(np.log2(np.maximum(v6, 1))).astype(np.int64)      # get_msb; exact here, v6 < 2^40
    i = np.where(v6 > 0, np.minimum(msb, 12), 0)
    return np.where(var != 0, (strength * (4 + i) + 8) >> 4, 0)


def constrain(diff, threshold, damping):
    """threshold: array (per sample) or int"""
    thr = np.broadcast_to(np.asarray(threshold, np.int64), diff.shape)
    shift = np.maximum(0, damping - MSB[thr])
    a = np.abs(diff)
    return np.where(thr != 0, np.sign(diff) * np.minimum(a, np.maximum(0, thr - (a >> shift))), 0)


def padded(plane):
    h, w = plane.shape
    p = np.full((h + 2 * PAD, w + 2 * PAD), VERY_LARGE, np.int64)
    p[PAD:PAD + h, PAD:PAD + w] = plane
    return p


def upsample(blocks, size):
    return np.repeat(np.repeat(blocks, size, 0), size, 1)


def filter_plane(plane, dirs, variances, listed, pli, level, sec_strength, pri_damping, sec_damping, shift, stats=None):
    """cdef_filter_fb's filtering arm on every 8x8 (luma) or 4x4 (chroma) block of a plane: level and sec_strength as cdef_filter_fb gets
    them.  -> the filtered plane (every block filtered; the caller keeps the listed ones)"""
    h, w = plane.shape
    size = 4 if pli else 8
    t = level << shift
    s = sec_strength << shift
    pd, sd = pri_damping + shift - (pli != 0), sec_damping + shift - (pli != 0)
    pri_b = np.full(dirs.shape, t, np.int64) if pli else adjust_strength(t, variances)
    dir_b = dirs if t else np.zeros_like(dirs)
    pri, dmap, lmap = upsample(pri_b, size), upsample(dir_b, size), upsample(listed, size)
    P = padded(plane)
    yy, xx = np.mgrid[0:h, 0:w]
    x = plane.astype(np.int64)
    tapsel = (pri >> shift) & 1
    total = np.zeros((h, w), np.int64)
    mx, mn = x.copy(), x.copy()
    off = np.array(DIRECTIONS, np.int64)      # [dir][k][row / column]
    sides = [0, 0, 0, 0]
    for k in range(2):
        for which, dd, thr, damp, tap in ((0, 0, pri, pd, None), (1, 2, s, sd, SEC_TAPS[k]), (1, 6, s, sd, SEC_TAPS[k])):
            d = (dmap + dd) & 7
            oy, ox = off[d, k, 0], off[d, k, 1]
            wgt = PRI_TAPS[tapsel, k] if which == 0 else tap
            for sgn in (1, -1):
                ty, tx = yy + sgn * oy, xx + sgn * ox
                v = P[ty + PAD, tx + PAD]
                total += wgt * constrain(v - x, thr, damp)
                mx = np.where(v != VERY_LARGE, np.maximum(v, mx), mx)
                mn = np.minimum(v, mn)
                if stats is not None:
                    for i, m in enumerate((ty < 0, tx < 0, ty >= h, tx >= w)):
                        sides[i] += int((m & lmap).sum())
    raw = x + ((8 + total - (total < 0)) >> 4)
    y = np.clip(raw, mn, mx)
    if stats is not None:
        for i, k in enumerate(("border_top", "border_left", "border_bottom", "border_right")):
            stats[k] += sides[i]
        stats["clamp_min"] += int(((raw < mn) & lmap).sum())
        stats["clamp_max"] += int(((raw > mx) & lmap).sum())
        if t == 0 and s:
            stats["pri0_sec"] += int(listed.sum())
        if t:
            stats["adj0"] += int(((pri_b == 0) & listed).sum())
            nz = listed & (pri_b != 0)
            stats["taps0"] += int((nz & (((pri_b >> shift) & 1) == 0)).sum())
            stats["taps1"] += int((nz & (((pri_b >> shift) & 1) == 1)).sum())
            if pli == 0:
                for d in range(8):
                    stats[f"dir{d}"] += int(((dirs == d) & listed).sum())
    return y


# ---------------------------------------------------------------- distortion
def dist_8x8(dst, src, shift):
    """dist_8x8_16bit_c on arrays of blocks [..., 64] -> uint64 [...]"""
    d, s = dst.astype(np.uint64), src.astype(np.uint64)
    sum_s, sum_d = s.sum(-1, dtype=np.uint64), d.sum(-1, dtype=np.uint64)
    sum_s2, sum_d2, sum_sd = (s * s).sum(-1, dtype=np.uint64), (d * d).sum(-1, dtype=np.uint64), (s * d).sum(-1, dtype=np.uint64)
    svar = sum_s2 - ((sum_s * sum_s + np.uint64(32)) >> np.uint64(6))
    dvar = sum_d2 - ((sum_d * sum_d + np.uint64(32)) >> np.uint64(6))
    sse = (sum_d2 + sum_s2 - np.uint64(2) * sum_sd).astype(np.float64)
    a = sse * .5
    a = a * (svar + dvar + np.uint64(400 << 2 * shift)).astype(np.float64)
    root = np.sqrt(np.float64(20000 << 4 * shift) + svar.astype(np.float64) * dvar.astype(np.float64))
    return np.floor(.5 + a / root).astype(np.uint64)


def blocks_of(plane, size):
    h, w = plane.shape
    return plane.reshape(h // size, size, w // size, size).transpose(0, 2, 1, 3).reshape(h // size, w // size, size * size)


def plane_dist(y, src, listed, pli, shift, nv, nh):
    """compute_cdef_dist of every fb: [nv][nh] uint64"""
    if pli == 0:
        b = dist_8x8(blocks_of(y, 8), blocks_of(src, 8), shift)
    else:
        e = blocks_of(y, 4).astype(np.int64) - blocks_of(src, 4).astype(np.int64)
        b = (e * e).sum(-1).astype(np.uint64)
    b = np.where(listed, b, np.uint64(0))
    return per_fb(b, nv, nh) >> np.uint64(2 * shift)


# ---------------------------------------------------------------- the search
def search(dbk, src, skip, w, h, bd, base_qindex, stats=None):
    """cdef_seg_search[16bit] over all fbs -> mse [2][nfb][64] uint64, counted [nfb] uint8, dirs, variances [h / 8][w / 8]"""
    shift = bd - 8
    nh, nv = geometry(w, h)
    listed, counted = block_lists(skip, w, h)
    damping = 3 + (base_qindex >> 6)
    dirs, variances = find_dirs(dbk[0], shift)
    mse = np.zeros((2, nv * nh, 64), np.uint64)
    for pli in range(3):
        for gi in range(64):
            level, sec = gi // 4, gi % 4
            if gi == 0:     # the dirinit arm: a copy
                y = dbk[pli].astype(np.int64)
                if stats is not None:
                    stats["copy"] += int(listed.sum())
            else:
                y = filter_plane(dbk[pli], dirs, variances, listed, pli, level, sec + (sec == 3), damping, damping, shift, stats)
            mse[min(pli, 1), :, gi] += plane_dist(y, src[pli], listed, pli, shift, nv, nh).reshape(-1)
    mse[:, ~counted.reshape(-1), :] = 0
    return mse, counted.reshape(-1).astype(np.uint8), dirs, variances


# ---------------------------------------------------------------- the pick
TOP = 1 << 63


def search_one_dual(lev0, lev1, nb, m0, m1):
    """search_one_dual_c: m0, m1 [sb_count][64] uint64 -> best total; writes lev0[nb], lev1[nb].  The totals stay far below 2^63, so
    uint64 sums are the reference's; argmin returns the first minimum in row-major (j, k) order, which is what its strict < keeps."""
    best = np.full(len(m0), TOP, np.uint64)
    for g in range(nb):
        best = np.minimum(best, m0[:, lev0[g]] + m1[:, lev1[g]])
    tot = np.minimum(m0[:, :, None] + m1[:, None, :], best[:, None, None]).sum(0, dtype=np.uint64)
    at = int(np.argmin(tot))
    lev0[nb], lev1[nb] = at // 64, at % 64
    return int(tot.reshape(-1)[at])


def joint_strength_search_dual(nb, m0, m1):
    lev0, lev1 = [0] * 16, [0] * 16
    best = TOP
    for i in range(nb):
        best = search_one_dual(lev0, lev1, i, m0, m1)
    for i in range(4 * nb):
        for j in range(nb - 1):
            lev0[j], lev1[j] = lev0[j + 1], lev1[j + 1]
        best = search_one_dual(lev0, lev1, nb - 1, m0, m1)
    return best, lev0, lev1


def pick(mse, counted, base_qindex, bd, lam=None):
    """finish_cdef_search -> result (RESULT_DTYPE scalar), fb_strength [nfb] int8 (-1: left out)"""
    lam = cdef_lambda(base_qindex, bd) if lam is None else lam
    idx = [i for i in range(len(counted)) if counted[i]]
    m0, m1 = np.asarray(mse[0], np.uint64)[idx].reshape(-1, 64), np.asarray(mse[1], np.uint64)[idx].reshape(-1, 64)
    sb_count = len(idx)
    best_tot, bits, s0, s1 = TOP, 0, [0] * 8, [0] * 8
    for i in range(4):
        nb = 1 << i
        tot, lev0, lev1 = joint_strength_search_dual(nb, m0, m1)
        tot += int(sb_count * lam * i)
        tot += int(nb * lam * 6)
        if tot < best_tot:
            best_tot, bits = tot, i
            s0[:nb], s1[:nb] = lev0[:nb], lev1[:nb]
    nb = 1 << bits
    res = np.zeros((), RESULT_DTYPE)
    res["cdef_bits"], res["nb_cdef_strengths"], res["sb_count"] = bits, nb, sb_count
    res["cdef_strengths"][:nb], res["cdef_uv_strengths"][:nb] = s0[:nb], s1[:nb]
    res["pri_damping"] = res["sec_damping"] = 3 + (base_qindex >> 6)
    fbs = np.full(len(counted), -1, np.int8)
    for n, i in enumerate(idx):
        best, bg = TOP, 0
        for g in range(nb):
            cur = int(m0[n][s0[g]]) + int(m1[n][s1[g]])
            if cur < best:
                best, bg = cur, g
        fbs[i] = bg
    return res, fbs


# ---------------------------------------------------------------- the frame filter
def frame(dbk, skip, w, h, bd, res, fb_strength, stats=None):
    """av1_cdef_frame[16bit] -> the three CDEF'd planes"""
    shift = bd - 8
    nh, nv = geometry(w, h)
    listed, _ = block_lists(skip, w, h)
    dirs, variances = find_dirs(dbk[0], shift)
    out = [p.copy() for p in dbk]
    groups = {}
    for fb in range(nv * nh):
        r, c = fb // nh, fb % nh
        g = max(int(fb_strength[fb]), 0)
        ys, uvs = int(res["cdef_strengths"][g]), int(res["cdef_uv_strengths"][g])
        if ys == 0 and uvs == 0:
            if stats is not None:
                stats["frame_zero_pair"] += 1
            continue
        if not listed[r * 8:(r + 1) * 8, c * 8:(c + 1) * 8].any():
            if stats is not None:
                stats["frame_empty_list"] += 1
            continue
        if stats is not None:
            stats["frame_filtered"] += 1
        groups.setdefault((ys, uvs), []).append((r, c))
    for (ys, uvs), fbs in groups.items():
        mask = np.zeros_like(listed)
        for (r, c) in fbs:
            mask[r * 8:(r + 1) * 8, c * 8:(c + 1) * 8] = listed[r * 8:(r + 1) * 8, c * 8:(c + 1) * 8]
        for pli in range(3):
            st = uvs if pli else ys
            sec = st % 4
            y = filter_plane(dbk[pli], dirs, variances, mask, pli, st // 4, sec + (sec == 3), int(res["pri_damping"]), int(res["sec_damping"]), shift, stats)
            m = upsample(mask, 4 if pli else 8)
            out[pli][m] = y[m].astype(out[pli].dtype)
    return out


# ---------------------------------------------------------------- the fixture
def fixture_path():
    return os.path.join(ROOT, "tests", "golden", "cdef.npz")


def load_case(z, c):
    w, h, bd = (int(v) for v in z["case"][c])
    dt = np.uint16 if bd > 8 else np.uint8
    src = [z[f"c{c}_src_{p}"] for p in range(3)]
    dbk = [(src[p].astype(np.int32) + z[f"c{c}_dbk_d{p}"]).astype(dt) for p in range(3)]
    F = {"w": w, "h": h, "bd": bd, "src": src, "dbk": dbk, "skip": z[f"c{c}_skip"], "qindex": [int(q) for q in z[f"c{c}_qindex"]],
         "mse": z[f"c{c}_mse"], "counted": z[f"c{c}_counted"], "result": z[f"c{c}_result"].view(RESULT_DTYPE).reshape(-1),
         "fb_strength": z[f"c{c}_fb_strength"], "dir_fb": int(z[f"c{c}_dir_fb"]), "dirs": z[f"c{c}_dirs"], "vars": z[f"c{c}_vars"],
         "run_result": z[f"c{c}_run_result"].view(RESULT_DTYPE).reshape(-1), "run_fb_strength": z[f"c{c}_run_fb_strength"]}
    F["nhfb"], F["nvfb"] = geometry(w, h)
    F["out"] = [[(dbk[p].astype(np.int32) + z[f"c{c}_out{r}_d{p}"]).astype(dt) for p in range(3)] for r in range(len(F["run_result"]))]
    return F
