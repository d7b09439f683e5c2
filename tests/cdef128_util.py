"""Restatement of what the reference's CDEF does with 128-wide blocks (cdef_seg_search[16bit] EbCdefProcess.c:157-246 / :249-410,
sb_all_skip / sb_compute_cdef_list EbCdef.c:359-428, compute_cdef_dist :1376-1425, finish_cdef_search :1471-1503 and :1535-1573,
av1_cdef_frame :565-570) on top of tests/cdef_util.py, whose per-block filter and distortion it uses.  With T the sb_type of an fb's first
cell: the fb is left out as a twin by its own cell, otherwise its extent is one or two fbs each way, clipped by the picture; it is left out
as all skipped by its first 64x64 alone; the distortions of every listed 8x8 block of the extent are summed and shifted once per plane;
the pick compacts the searched fbs, and afterwards each pick goes to its own fb and to the other fbs of its block, in raster order.
Also the cases of tests/golden/cdef128.npz (make_golden_cdef128.py writes it) and its loader."""
import os

import numpy as np

import cdef_util as cu

BLOCK_8X8, BLOCK_16X16, BLOCK_32X32, BLOCK_64X64, BLOCK_64X128, BLOCK_128X64, BLOCK_128X128 = 3, 6, 9, 12, 13, 14, 15   # BlockSize
QINDEX = (20, 100, 255)
# name, width, height; every one at 8 and at 10 bits.  E is not in the issue's list: no fb of A-D can drop a copy (their fb counts are even
# each way, so an fb in the last column or row that names a wide type is a twin), E's 3 x 3 fbs can.
CASES = tuple((n, w, h, bd) for bd in (8, 10) for (n, w, h) in (("A", 128, 128), ("B", 328, 200), ("C", 128, 128), ("D", 328, 200), ("E", 136, 136)))
COVERAGE_KEYS = ("type_128x128", "type_128x64", "type_64x128", "wide_full", "wide_clipped_right", "wide_clipped_bottom", "twin_by_column", "twin_by_row",
                 "first_quadrant_skipped_others_listed", "single_block_in_first_quadrant", "other_quadrant_skipped", "shift_once_differs_10bit",
                 "pick_differs_from_64x64", "copy_dropped", "copy_order_decides")


def fixture_path():
    return os.path.join(cu.ROOT, "tests", "golden", "cdef128.npz")


# ---------------------------------------------------------------- the grid
def shapes(sb_type, w, h):
    """-> wide, tall [nvfb][nhfb] bool from the sb_type of each fb's first cell (values above 21 clamped, as the device does)"""
    nh, nv = cu.geometry(w, h)
    t = np.minimum(np.asarray(sb_type)[0:nv * 16:16, 0:nh * 16:16].astype(np.int64), 21)
    return (t == BLOCK_128X128) | (t == BLOCK_128X64), (t == BLOCK_128X128) | (t == BLOCK_64X128)


def layout(sb_type, skip, w, h):
    """-> searched [nv][nh] bool, twin [nv][nh] bool, nx, ny [nv][nh] (the extent in fbs, clipped by the picture)"""
    nh, nv = cu.geometry(w, h)
    wide, tall = shapes(sb_type, w, h)
    r, c = np.mgrid[0:nv, 0:nh]
    twin = (((c & 1) == 1) & wide) | (((r & 1) == 1) & tall)
    _, first = cu.block_lists(skip, w, h)          # sb_all_skip looks at the first 64x64 only
    nx = np.where(wide & (c + 1 < nh), 2, 1)
    ny = np.where(tall & (r + 1 < nv), 2, 1)
    return first & ~twin, twin, nx, ny


# ---------------------------------------------------------------- the search
def quadrant_sums(dbk, src, skip, w, h, bd, base_qindex):
    """unshifted sums of the listed blocks' distortions per 64x64 quadrant: [3 planes][nfb][64] uint64"""
    shift = bd - 8
    nh, nv = cu.geometry(w, h)
    listed, _ = cu.block_lists(skip, w, h)
    damping = 3 + (base_qindex >> 6)
    dirs, variances = cu.find_dirs(dbk[0], shift)
    out = np.zeros((3, nv * nh, 64), np.uint64)
    for pli in range(3):
        for gi in range(64):
            sec = gi % 4
            y = dbk[pli].astype(np.int64) if gi == 0 else cu.filter_plane(dbk[pli], dirs, variances, listed, pli, gi // 4, sec + (sec == 3), damping, damping, shift)
            if pli == 0:
                b = cu.dist_8x8(cu.blocks_of(y, 8), cu.blocks_of(src[pli], 8), shift)
            else:
                e = cu.blocks_of(y, 4).astype(np.int64) - cu.blocks_of(src[pli], 4).astype(np.int64)
                b = (e * e).sum(-1).astype(np.uint64)
            out[pli, :, gi] = cu.per_fb(np.where(listed, b, np.uint64(0)), nv, nh).reshape(-1)
    return out


def merge(quads, sb_type, skip, w, h, bd):
    """the tables from the quadrants' sums -> mse [2][nfb][64], counted [nfb] uint8"""
    nh, nv = cu.geometry(w, h)
    s = np.uint64(2 * (bd - 8))
    searched, _, nx, ny = layout(sb_type, skip, w, h)
    mse = np.zeros((2, nv * nh, 64), np.uint64)
    for r in range(nv):
        for c in range(nh):
            if searched[r, c]:
                tot = np.zeros((3, 64), np.uint64)
                for dy in range(ny[r, c]):
                    for dx in range(nx[r, c]):
                        tot += quads[:, (r + dy) * nh + c + dx, :]
                mse[0, r * nh + c], mse[1, r * nh + c] = tot[0] >> s, (tot[1] >> s) + (tot[2] >> s)
    return mse, searched.reshape(-1).astype(np.uint8)


def search(dbk, src, skip, sb_type, w, h, bd, base_qindex):
    return merge(quadrant_sums(dbk, src, skip, w, h, bd, base_qindex), sb_type, skip, w, h, bd)


# ---------------------------------------------------------------- the pick
def spread(own, counted, sb_type, w, h):
    """finish_cdef_search's writes in its order: own [nfb] (the picks of the counted fbs) -> fb_strength [nfb], dropped copies, and whether a
    later write changed an entry an earlier one had set"""
    nh, nv = cu.geometry(w, h)
    wide, tall = shapes(sb_type, w, h)
    out = np.full(nh * nv, -1, np.int8)
    dropped, overwritten = 0, False
    for fb in np.flatnonzero(counted):
        r, c = fb // nh, fb % nh
        for (dy, dx) in ((0, 0), (0, 1), (1, 0), (1, 1)):
            if (dx and not wide[r, c]) or (dy and not tall[r, c]):
                continue
            if r + dy >= nv or c + dx >= nh:
                dropped += 1
                continue
            at = (r + dy) * nh + c + dx
            overwritten |= out[at] >= 0 and out[at] != own[fb]
            out[at] = own[fb]
    return out, dropped, overwritten


def pick(mse, counted, sb_type, w, h, base_qindex, bd):
    """-> result (sb_count = the searched fbs), fb_strength [nfb] int8"""
    res, own = cu.pick(mse, counted, base_qindex, bd)
    return res, spread(own, counted, sb_type, w, h)[0]


# ---------------------------------------------------------------- the frame filter
def frame(dbk, skip, w, h, bd, res, fb_strength):
    """av1_cdef_frame[16bit]: 64x64 fbs, each with the index of its first cell; an fb whose index is -1 is passed over"""
    nh, nv = cu.geometry(w, h)
    masked = np.array(skip, np.uint8, copy=True)
    for fb in np.flatnonzero(np.asarray(fb_strength) < 0):
        r, c = fb // nh, fb % nh
        masked[r * 16:(r + 1) * 16, c * 16:(c + 1) * 16] = 1      # nothing listed: passed over
    return cu.frame(dbk, masked, w, h, bd, res, fb_strength)


# ---------------------------------------------------------------- the cases
def make_grid(name, w, h):
    """sb_type per 4x4 cell [h / 4][w / 4]"""
    mr, mc = h >> 2, w >> 2
    g = np.full((mr, mc), BLOCK_16X16, np.uint8)

    def put(r0, c0, rows, cols, t):
        g[r0:r0 + rows, c0:c0 + cols] = t

    if name == "A":
        put(0, 0, 32, 32, BLOCK_128X128)
    elif name == "B":
        put(0, 0, 32, 32, BLOCK_128X128)       # superblock (0, 0)
        put(0, 32, 16, 32, BLOCK_128X64)       # (1, 0): over two 64x64 areas of small blocks
        put(16, 32, 16, 32, BLOCK_8X8)
        put(0, 64, 32, 16, BLOCK_64X128)       # (2, 0): fb column 4, small blocks in column 5
        put(0, 80, 32, 2, BLOCK_8X8)
        put(32, 0, 18, 32, BLOCK_128X128)      # (0, 1): clipped at the bottom
        put(32, 32, 16, 32, BLOCK_128X64)      # (1, 1): fb row 2 over small blocks in row 3
        put(48, 32, 2, 32, BLOCK_8X8)
        put(32, 64, 18, 18, BLOCK_128X128)     # (2, 1): clipped both ways
    elif name == "C":                          # contradictory: the first cells say 128X128, 64X64, 128X64, 64X64
        put(0, 0, 16, 16, BLOCK_128X128), put(0, 16, 16, 16, BLOCK_64X64), put(16, 0, 16, 16, BLOCK_128X64), put(16, 16, 16, 16, BLOCK_64X64)
    elif name == "D":                          # B's picture with nothing 128 wide
        put(0, 0, 32, 32, BLOCK_64X64), put(32, 0, 18, 32, BLOCK_32X32)
    elif name == "E":                          # 3 x 3 fbs, the last 8 samples: 128X128 everywhere, so copies leave the picture
        put(0, 0, mr, mc, BLOCK_128X128)
    return g


def make_skip(rng, name, w, h):
    mr, mc = h >> 2, w >> 2
    if name in ("A", "C"):
        return np.zeros((mr, mc), np.uint8)
    skip = (rng.random((mr, mc)) < 0.55).astype(np.uint8)
    if name in ("B", "D"):
        skip[0, 0] = 0
        skip[0:16, 16:32] = 1                  # (0, 0): the first quadrant listed, the second one skipped
        skip[32:50, 0:32] = 1                  # (0, 1): a single listed block, inside the first quadrant
        skip[35, 9] = 0
        skip[32:48, 32:48] = 1                 # (1, 1): the first 64x64 all skipped, its twin not
        skip[33, 50] = 0
    return skip


def load_case(z, c):
    name, w, h, bd = str(z["case_name"][c]), *(int(v) for v in z["case"][c])
    dt = np.uint16 if bd > 8 else np.uint8
    p = int(z["case_picture"][c])               # the case whose planes and skip map this one shares
    src = [z[f"c{p}_src_{i}"] for i in range(3)]
    dbk = [(src[i].astype(np.int32) + z[f"c{p}_dbk_d{i}"]).astype(dt) for i in range(3)]
    F = {"name": name, "w": w, "h": h, "bd": bd, "src": src, "dbk": dbk, "skip": z[f"c{p}_skip"], "sb_type": z[f"c{c}_sb_type"],
         "qindex": [int(q) for q in z["qindex"]], "mse": z[f"c{c}_mse"], "counted": z[f"c{c}_counted"],
         "result": z[f"c{c}_result"].view(cu.RESULT_DTYPE).reshape(-1), "fb_strength": z[f"c{c}_fb_strength"],
         "run_result": z[f"c{c}_run_result"].view(cu.RESULT_DTYPE).reshape(-1), "run_fb_strength": z[f"c{c}_run_fb_strength"]}
    F["nhfb"], F["nvfb"] = cu.geometry(w, h)
    F["out"] = [[(dbk[i].astype(np.int32) + z[f"c{c}_out{r}_d{i}"]).astype(dt) for i in range(3)] for r in range(len(F["run_result"]))]
    return F


def coverage(cases, quads=None):
    """cases: dicts as load_case gives them; quads(F): quadrant_sums at qindex[0] where the caller has them -> {key: bool} of COVERAGE_KEYS"""
    f = {k: False for k in COVERAGE_KEYS}
    for F in cases:
        w, h, bd, nh, nv = F["w"], F["h"], F["bd"], F["nhfb"], F["nvfb"]
        searched, twin, nx, ny = layout(F["sb_type"], F["skip"], w, h)
        wide, tall = shapes(F["sb_type"], w, h)
        listed, first = cu.block_lists(F["skip"], w, h)
        per = cu.per_fb(listed.astype(np.int64), nv, nh)
        r, c = np.mgrid[0:nv, 0:nh]
        own = ~twin                                 # fbs asked on their own
        f["type_128x128"] |= bool((own & wide & tall).any())
        f["type_128x64"] |= bool((own & wide & ~tall).any())
        f["type_64x128"] |= bool((own & ~wide & tall).any())
        f["wide_full"] |= bool((own & wide & tall & (16 * c + 32 <= w // 4) & (16 * r + 32 <= h // 4)).any())
        f["wide_clipped_right"] |= bool((own & wide & (16 * c + 32 > w // 4) & (nx == 2)).any())
        f["wide_clipped_bottom"] |= bool((own & tall & (16 * r + 32 > h // 4) & (ny == 2)).any())
        f["twin_by_column"] |= bool((((c & 1) == 1) & wide & ~(((r & 1) == 1) & tall)).any())
        f["twin_by_row"] |= bool((((r & 1) == 1) & tall & ~(((c & 1) == 1) & wide)).any())
        for fr in range(nv):
            for fc in range(nh):
                if twin[fr, fc] or nx[fr, fc] * ny[fr, fc] == 1:
                    continue
                ext = per[fr:fr + ny[fr, fc], fc:fc + nx[fr, fc]]
                f["first_quadrant_skipped_others_listed"] |= bool(not first[fr, fc] and ext.sum() > 0)
                f["single_block_in_first_quadrant"] |= bool(ext.sum() == 1 and per[fr, fc] == 1)
                f["other_quadrant_skipped"] |= bool(per[fr, fc] > 0 and (ext == 0).any())
        q0 = quads(F) if quads else quadrant_sums(F["dbk"], F["src"], F["skip"], w, h, bd, F["qindex"][0])
        mse64, counted64 = merge(q0, np.full_like(F["sb_type"], BLOCK_64X64), F["skip"], w, h, bd)     # the existing 64x64 treatment
        if bd == 10:                                # 10 bits: the sum of the quadrants' shifted sums against the shifted sum
            for fb in np.flatnonzero(F["counted"]):
                fr, fc = fb // nh, fb % nh
                if nx[fr, fc] * ny[fr, fc] > 1:
                    q = [(fr + dy) * nh + fc + dx for dy in range(ny[fr, fc]) for dx in range(nx[fr, fc])]
                    f["shift_once_differs_10bit"] |= not np.array_equal(mse64[:, q, :].sum(1, dtype=np.uint64), F["mse"][0][:, fb, :])
        res64, fbs64 = cu.pick(mse64, counted64, F["qindex"][0], bd)
        got = F["result"][0]
        f["pick_differs_from_64x64"] |= int(res64["sb_count"]) != int(got["sb_count"]) and any(
            not np.array_equal(res64[k], got[k]) for k in ("cdef_bits", "cdef_strengths", "cdef_uv_strengths"))
        for qi in range(len(F["qindex"])):
            _, own_picks = cu.pick(F["mse"][qi], F["counted"], F["qindex"][qi], bd)
            _, dropped, over = spread(own_picks, F["counted"], F["sb_type"], w, h)
            f["copy_dropped"] |= dropped > 0
            f["copy_order_decides"] |= bool(over) and F["name"] == "C"
    return f
