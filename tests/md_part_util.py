"""Mode decision's partition decision, restated in numpy / plain Python for the tests: the block table of the md scan (our own recursion),
the lists of the reference's four forward_* functions built from their rules, the serial walk of mode_decision_sb's loop (d1, d2 with
its quirks), EncodePass's walk and the composition of the winner tiles.  It is the checker of the GPU tests, where the reference is
absent; tests/test_md_part_vs_ref.py holds it to tests/golden/md_part.npz and to the live reference driver.

A case is one picture: 136x72 with 64x64 superblocks ("p64": 3 x 2 superblocks, the right column and the bottom row 8 wide / high) or
264x136 with 128x128 superblocks ("p128"), one list kind, intra or inter, one cost variant.  Everything of a case but the reference's
results is made here from its name, so the fixture holds digests and the short final lists only."""
import ctypes as C
import functools
import hashlib
import os
import zlib

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MAX_MODE_COST = 13616969489728 * 8
M64 = (1 << 64) - 1
NONE = 0xFFFFFFFF
SPLIT = 3
PICTURES = {"p64": (136, 72, 64), "p128": (264, 136, 128)}
KINDS = ("all", "all_c", "sq", "sq_non4")
POOL_W = 2048

# the blocks of a shape in quarters of the square: (x, y, w, h)
SHAPE_RECTS = (
    ((0, 0, 4, 4),),
    ((0, 0, 4, 2), (0, 2, 4, 2)),
    ((0, 0, 2, 4), (2, 0, 2, 4)),
    ((0, 0, 2, 2), (2, 0, 2, 2), (0, 2, 4, 2)),
    ((0, 0, 4, 2), (0, 2, 2, 2), (2, 2, 2, 2)),
    ((0, 0, 2, 2), (0, 2, 2, 2), (2, 0, 2, 4)),
    ((0, 0, 2, 4), (2, 0, 2, 2), (2, 2, 2, 2)),
    tuple((0, k, 4, 1) for k in range(4)),
    tuple((k, 0, 1, 4) for k in range(4)),
)
SHAPE_START = (0, 1, 3, 5, 8, 11, 14, 17, 21)
PART_OF_SHAPE = (0, 1, 2, 4, 5, 6, 7, 8, 9)          # from_shape_to_part
SHAPE_OF_PART = {p: s for s, p in enumerate(PART_OF_SHAPE)}
GEOM_DTYPE = np.dtype([("origin_x", "u1"), ("origin_y", "u1"), ("bwidth", "u1"), ("bheight", "u1"), ("shape", "u1"), ("depth", "u1"), ("nsi", "u1"),
                       ("totns", "u1"), ("sqi_mds", "<u2"), ("parent_mds", "<u2"), ("is_last_quadrant", "u1"), ("has_uv", "u1"), ("bwidth_uv", "u1"),
                       ("bheight_uv", "u1")])
SB_DTYPE = np.dtype([("first_leaf", "<u4"), ("leaf_count", "<u4"), ("full_lambda", "<u4"), ("origin_x", "<u2"), ("origin_y", "<u2")])
LEAF_DTYPE = np.dtype([("decision_index", "<u4"), ("mds_idx", "<u2"), ("tot_d1_blocks", "u1"), ("split_flag", "u1"), ("pool_x", "<u2"), ("pool_y", "<u2"),
                       ("reserved", "u1", (4,))])
RESULT_DTYPE = np.dtype([("cost", "<u8"), ("leaf", "<u4"), ("best_d1_blk", "<u2"), ("part", "u1"), ("flags", "u1")])
FINAL_DTYPE = np.dtype([("leaf", "<u4"), ("mds_idx", "<u2"), ("x", "<u2"), ("y", "<u2"), ("bwidth", "u1"), ("bheight", "u1"), ("has_uv", "u1"), ("part", "u1"),
                        ("n_part", "u1"), ("reserved", "u1")])
DECISION_DTYPE = np.dtype([("cost", "<u8"), ("winner_row", "<u4"), ("winner_slot", "u1"), ("winner_buffer", "u1"), ("best_intra_mode", "u1"), ("n_full", "u1")])


def n_shapes(size):
    return 7 if size == 128 else 3 if size == 8 else 1 if size == 4 else 9


def subtree(size):
    return 1 if size == 4 else SHAPE_START[n_shapes(size) - 1] + len(SHAPE_RECTS[n_shapes(size) - 1]) + 4 * subtree(size // 2)


def _scan(out, size, x, y, last, depth, parent):
    sq, q = len(out), size // 4
    for shape in range(n_shapes(size)):
        for nsi, (qx, qy, qw, qh) in enumerate(SHAPE_RECTS[shape]):
            w, h = q * qw, q * qh
            if w == 4 and h == 4:
                has_uv = last
            elif w == 4 or h == 4:   # 2 luma blocks share a chroma block: it goes with the second (and the fourth)
                has_uv = nsi in (1, 3)
            else:
                has_uv = 1
            out.append((x + q * qx, y + q * qy, w, h, shape, depth, nsi, len(SHAPE_RECTS[shape]), sq, parent, last, has_uv, max(4, w // 2), max(4, h // 2)))
    if size > 4:
        half = size // 2
        for k in range(4):
            _scan(out, half, x + (k & 1) * half, y + (k >> 1) * half, int(k == 3), depth + 1, sq)


@functools.lru_cache(maxsize=None)
def geometry(sb_size):
    out = []
    _scan(out, sb_size, 0, 0, 0, 0, 0xFFFF)
    return np.array(out, GEOM_DTYPE)


def sb_origins(w, h, sb):
    return [(x, y) for y in range(0, h, sb) for x in range(0, w, sb)]


def inside(sb_size, ox, oy, w, h):
    """block_is_inside_md_scan: a block is in when its SQUARE lies inside the picture"""
    g = geometry(sb_size)
    sq = g[g["sqi_mds"]]
    return (ox + sq["origin_x"].astype(int) + sq["bwidth"] <= w) & (oy + sq["origin_y"].astype(int) + sq["bheight"] <= h)


def leaf_list(kind, sb_size, ins, intra):
    """[(mds_idx, tot_d1_blocks, split_flag)] of forward_all_blocks_to_md / forward_all_c_blocks_to_md / forward_sq_blocks_to_md /
    forward_sq_non4_blocks_to_md (Codec/EbModeDecisionConfigurationProcess.c:926-1055, :2477-2599) for one superblock"""
    g = geometry(sb_size)
    n = len(g)
    size = lambda i: sb_size >> int(g["depth"][i])  # noqa: E731
    d1n = lambda z: SHAPE_START[n_shapes(z) - 1] + len(SHAPE_RECTS[n_shapes(z) - 1])  # noqa: E731
    out, i = [], 0
    if kind == "all":
        for i in range(n):
            z = size(i)
            if ins[i] and not (intra and z == 128):
                out.append((i, 17 if z == 128 else 25 if z > 8 else 5 if z == 8 else 1, int(z > 4)))
    elif kind == "all_c":
        while i < n:
            z, tot = size(i), 0
            if ins[i] and not (intra and z == 128):
                tot = 17 if z == 128 else 25 if z > 16 else 17 if z == 16 else 1
                out += [(j, tot, int(z > 4)) for j in range(i, i + tot) if ins[j]]
            i += d1n(z)
    else:
        floor = 4 if kind == "sq" else 8
        i = 17 if intra and sb_size == 128 else 0
        while i < n:
            z, split = size(i), 1
            if ins[i]:
                split = int(z > floor)
                out.append((i, 1, split))
            i += d1n(z) if split else subtree(z)
    return out


def rate(fac, lam, size, split):
    row = 0 if size < 8 else 4 if size == 8 else 8 if size == 128 else 10
    return ((int(fac[row][SPLIT if split else 0]) * lam + 256) >> 9) & M64


def walk(sb_size, leaves, costs, lam, fac, intra, stats=None):
    """the loop of mode_decision_sb (Codec/EbProductCodingLoop.c:2762-2880) with md_encode_block replaced by the given costs, then
    EncodePass's walk.  Returns cost, part, split_flag, best_d1_blk, tested, mdc_split_flag per md-scan index and the final indices."""
    g = geometry(sb_size)
    n = len(g)
    shape, sqi, par, lastq, depth, nsi, totns = (g[k].tolist() for k in ("shape", "sqi_mds", "parent_mds", "is_last_quadrant", "depth", "nsi", "totns"))
    cost, best, tested, mdc = [MAX_MODE_COST] * n, [0] * n, [0] * n, [0] * n
    part = [SPLIT if s == 0 else 0 for s in shape]
    split = [1 if s == 0 else 0 for s in shape]
    st = stats if stats is not None else {}
    acc = 0
    for (m, tot_d1, sf), c in zip(leaves, costs):
        tested[m], mdc[m], split[m], best[m], cost[m] = 1, sf, sf, m, c
        sq = sqi[m]
        if nsi[m] + 1 == totns[m]:   # d1_non_square_block_decision
            first = m - (totns[m] - 1)
            tot = sum(cost[first:first + totns[m]]) & M64
            if shape[m] and tot == cost[sq]:
                st["d1_ties"] = st.get("d1_ties", 0) + 1
            if shape[m] == 0 or tot < cost[sq]:
                cost[sq], part[sq], best[sq] = tot, PART_OF_SHAPE[shape[m]], first
        acc = 1 if shape[m] == 0 else acc + 1
        if acc != tot_d1 or split[sq]:
            continue
        big = (int(g["bwidth"][m]), int(g["bheight"][m])) != (4, 4)   # context_ptr->blk_geom is the leaf's
        cur, parent_cost, current_cost = sq, 0, 0
        while lastq[cur]:
            p, z = par[cur], sb_size >> depth[cur]
            step = subtree(z)
            if intra and p == 0:
                parent_cost = MAX_MODE_COST
                if current_cost:
                    st["stale_root"] = st.get("stale_root", 0) + 1
            else:
                parent_cost = (cost[p] + rate(fac, lam, 2 * z, 0)) & M64 if tested[p] else MAX_MODE_COST
                current_cost = rate(fac, lam, 2 * z, 1)
                for k in range(4):
                    child = cur - k * step
                    current_cost += cost[child] + (rate(fac, lam, z, 0) if big and not mdc[child] else 0)
                current_cost &= M64
                if parent_cost == current_cost:
                    st["d2_ties"] = st.get("d2_ties", 0) + 1
            if parent_cost <= current_cost:
                split[p], cost[p] = 0, parent_cost
            else:
                cost[p], part[p] = current_cost, SPLIT
            cur = p
    final, i = [], 0
    while i < n:
        z = sb_size >> depth[i]
        if part[i] != SPLIT:
            s = SHAPE_OF_PART[part[i]]
            final += list(range(i + SHAPE_START[s], i + SHAPE_START[s] + len(SHAPE_RECTS[s])))
            i += subtree(z)
        else:
            i += SHAPE_START[n_shapes(z) - 1] + len(SHAPE_RECTS[n_shapes(z) - 1])
    return {"cost": cost, "part": part, "split": split, "best": best, "tested": tested, "mdc": mdc, "final": final}


# ---------------------------------------------------------------- the cases

def _case_names():
    names = []
    for pic in PICTURES:
        names += [f"{pic}-{kind}-{sl}-v0" for kind in KINDS for sl in "ip"]
        names += [f"{pic}-all-p-v{v}" for v in range(1, 5)] + [f"{pic}-all-i-v1", f"{pic}-all_c-p-v1"]
        names += [f"{pic}-all-p-ties", f"{pic}-all-i-ties"]
    return names + ["p64-irregular-p-v0", "p64-leafless-p-v0"]


CASES = _case_names()


class Scenario:
    pass


def _special_lists(kind, sb_size, ins, sb_index):
    """two lists no forward_* function makes: "irregular" reaches tot_d1_blocks before the last listed block of the last 32x32 quadrant, so
    its d2 call sees the square's cost before the V shape is decided; "leafless" lets a shape win whose first block no leaf names"""
    base = leaf_list("sq", sb_size, ins, False)
    if sb_index != 0:
        return base, {}
    if kind == "irregular":
        q3 = 25 + 3 * 269
        leaves = [(0, 1, 1)] + [(25 + k * 269, 1, 0) for k in range(3)] + [(q3 + j, 3, 0) for j in range(5)]
        return leaves, {0: 500000, q3: 100000, q3 + 1: 30000, q3 + 2: 30000, q3 + 3: 9000, q3 + 4: 9000}
    return [(0, 3, 0), (2, 3, 0)], {0: 1000, 2: (1 << 64) - MAX_MODE_COST + 5}


@functools.lru_cache(maxsize=None)
def scenario(name):
    pic, kind, sl, variant = name.split("-")
    s = Scenario()
    s.name, (s.w, s.h, s.sb_size), s.intra, s.kind = name, PICTURES[pic], sl == "i", kind
    g = geometry(s.sb_size)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ties = variant == "ties"
    v = 0 if ties else int(variant[1:])
    s.fac = np.zeros((20, 11), np.int32) if ties else rng.integers(150, 3000, (20, 11)).astype(np.int32)
    s.origins = sb_origins(s.w, s.h, s.sb_size)
    s.lists, s.costs, s.lams = [], [], []
    counters = {}
    area = g["bwidth"].astype(np.int64) * g["bheight"]
    for k, (ox, oy) in enumerate(s.origins):
        ins = inside(s.sb_size, ox, oy, s.w, s.h)
        complete = ox + s.sb_size <= s.w and oy + s.sb_size <= s.h
        if kind in ("irregular", "leafless"):
            leaves, given = _special_lists(kind, s.sb_size, ins, k)
        else:
            leaves, given = leaf_list(kind, s.sb_size, ins, s.intra), {}
        factor = rng.integers(1, 3, len(g)) if ties else rng.integers(95, 106, len(g))
        favoured = {}
        for m in range(len(g)):   # a favoured shape per square, taken in turn per square size
            if g["shape"][m] == 0 and not ties:
                z = s.sb_size >> int(g["depth"][m])
                c = counters.get(z, 0)
                counters[z] = c + 1
                favoured[m] = (c + 2 * v) % (n_shapes(z) + 1)
        costs = []
        for m, _, _ in leaves:
            c = int(area[m]) * int(factor[m])
            if favoured.get(int(g["sqi_mds"][m]), -1) == int(g["shape"][m]):
                c = c * (6 if g["depth"][m] == 0 else 8) // 10   # a favoured shape of the root also beats its quadrants' favoured shapes
            if not complete and g["shape"][m]:
                c = None   # md_encode_block refuses a non-square block of an incomplete superblock: MAX_MODE_COST
            costs.append(given.get(m, c))
        if ties and k == 0:
            j = next(i for i, (m, _, _) in enumerate(leaves) if g["shape"][m] == 1 and g["bwidth"][m] == 16)
            costs[j] = M64   # a cost of ~0 in a listed shape: the sum wraps
        s.lists.append(leaves), s.costs.append(costs), s.lams.append(0 if ties else 60 + 7 * k)
    # the arrays of the call
    n_leaf = sum(len(x) for x in s.lists)
    s.sbs, s.leaves = np.zeros(len(s.origins), SB_DTYPE), np.zeros(n_leaf, LEAF_DTYPE)
    decisions, at, px, py, shelf = [], 0, 0, 0, 0
    for k, ((ox, oy), leaves, costs) in enumerate(zip(s.origins, s.lists, s.costs)):
        s.sbs[k] = (at, len(leaves), s.lams[k], ox, oy)
        for (m, tot, sf), c in zip(leaves, costs):
            pw, ph = max(8, int(g["bwidth"][m])), max(8, int(g["bheight"][m]))
            if px + pw > POOL_W:
                px, py, shelf = 0, py + shelf, 0
            shelf = max(shelf, ph)
            s.leaves[at] = (NONE if c is None else len(decisions), m, tot, sf, px, py, 0)
            if c is not None:
                decisions.append(c)
            px, at = px + pw, at + 1
    s.pool_w, s.pool_h = POOL_W, py + shelf
    s.decisions = np.zeros(len(decisions) + 3, DECISION_DTYPE)   # three rows nothing points at
    s.decisions["cost"][:len(decisions)] = np.array(decisions, np.uint64)
    s.decisions["winner_row"] = np.arange(len(s.decisions))
    s.pool = [rng.integers(0, 256, (s.pool_h, POOL_W), np.uint8), *(rng.integers(0, 256, ((s.pool_h + 1) // 2, POOL_W // 2), np.uint8) for _ in range(2))]
    return s


def leaf_costs(s, k):
    return [MAX_MODE_COST if c is None else c for c in s.costs[k]]


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restated call: result rows [n_sb][n_blocks], final rows [n_sb][max_final], counts, the refused count, the composed planes, and
    what the walk met (stats)"""
    s = scenario(name)
    g = geometry(s.sb_size)
    n, max_final = len(g), 1024 if s.sb_size == 128 else 256
    result, final = np.zeros((len(s.origins), n), RESULT_DTYPE), np.zeros((len(s.origins), max_final), FINAL_DTYPE)
    count, stats, refused, walks = np.zeros(len(s.origins), np.uint32), {}, 0, []
    dst = [np.full((s.h, s.w), 0xA5, np.uint8), *(np.full(((s.h + 1) // 2, (s.w + 1) // 2), 0xA5, np.uint8) for _ in range(2))]
    for k, (ox, oy) in enumerate(s.origins):
        r = walk(s.sb_size, s.lists[k], leaf_costs(s, k), s.lams[k], s.fac, s.intra, stats)
        walks.append(r)
        first = int(s.sbs["first_leaf"][k])
        leaf_of = {m: first + i for i, (m, _, _) in enumerate(s.lists[k])}
        result[k]["cost"], result[k]["best_d1_blk"], result[k]["part"] = np.array(r["cost"], np.uint64), r["best"], r["part"]
        result[k]["flags"] = np.array(r["split"]) * 1 + np.array(r["tested"]) * 2 + (np.array(r["mdc"]) != 0) * 4
        result[k]["leaf"] = [leaf_of.get(m, NONE) for m in range(n)]
        count[k] = len(r["final"])
        for j, m in enumerate(r["final"]):
            b, sq = g[m], int(g["sqi_mds"][m])
            final[k][j] = (leaf_of.get(m, NONE), m, ox + int(b["origin_x"]), oy + int(b["origin_y"]), b["bwidth"], b["bheight"], b["has_uv"], r["part"][sq],
                           len(SHAPE_RECTS[SHAPE_OF_PART[r["part"][sq]]]), 0)
            if m not in leaf_of:
                refused += 1
                continue
            compose_block(dst, s.pool, final[k][j], s.leaves[leaf_of[m]])
    return {"result": result, "final": final, "count": count, "refused": refused, "dst": dst, "stats": stats, "walks": walks}


def compose_block(dst, pool, f, leaf):
    x, y, w, h, px, py = int(f["x"]), int(f["y"]), int(f["bwidth"]), int(f["bheight"]), int(leaf["pool_x"]), int(leaf["pool_y"])
    dst[0][y:y + h, x:x + w] = pool[0][py:py + h, px:px + w]
    if f["has_uv"]:
        cw, ch = max(4, w // 2), max(4, h // 2)
        cx, cy, pcx, pcy = ((x >> 3) << 3) // 2, ((y >> 3) << 3) // 2, ((px >> 3) << 3) // 2, ((py >> 3) << 3) // 2
        for p in (1, 2):
            dst[p][cy:cy + ch, cx:cx + cw] = pool[p][pcy:pcy + ch, pcx:pcx + cw]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def state_digest(r):
    """one digest of what the reference's driver and the restatement both give per md-scan index"""
    return digest(np.array(r["cost"], np.uint64), np.array([r["part"], r["split"], r["best"], r["tested"], r["mdc"]], np.uint32))


def coverage(names):
    """what the issue asks the cases to hold, from the walks of `names`"""
    wins, splits, stats, max_shapes = {}, {}, {}, 0
    for name in names:
        s, e = scenario(name), expected(name)
        g = geometry(s.sb_size)
        for k, r in enumerate(e["walks"]):
            for m in np.nonzero(g["shape"] == 0)[0].tolist():
                if r["tested"][m]:
                    z = s.sb_size >> int(g["depth"][m])
                    wins.setdefault(z, set()).add(r["part"][m])
                    splits.setdefault(z, set()).add(r["part"][m] == SPLIT)
            max_shapes += sum(1 for (m, _, _), c in zip(s.lists[k], s.costs[k]) if c is None and g["shape"][m])
        for key, val in e["stats"].items():
            stats[key] = stats.get(key, 0) + val
    return wins, splits, stats, max_shapes


def assert_coverage(names):
    wins, splits, stats, max_shapes = coverage(names)
    for z, want in ((128, {0, 1, 2, 3, 4, 5, 6, 7}), (64, set(range(10))), (32, set(range(10))), (16, set(range(10))), (8, {0, 1, 2, 3}), (4, {0})):
        assert wins.get(z) == want, (z, wins.get(z))
    assert all(splits[z] == {True, False} for z in (128, 64, 32, 16, 8)), splits
    assert stats.get("d1_ties", 0) >= 1 and stats.get("d2_ties", 0) >= 1 and stats.get("stale_root", 0) >= 1, stats
    assert max_shapes >= 1
    return stats


# ---------------------------------------------------------------- the fixture and the live reference

@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "md_part.npz"))


def build_reference_driver(out_dir):
    from oracle import ref_driver
    L = ref_driver.build_driver(os.path.join(ROOT, "tests", "golden", "ref_md_part_driver.c"), out_dir)
    V, U = C.c_void_p, C.c_uint32
    L.drv_md_part_geometry.argtypes = [C.c_int, V]
    L.drv_md_part_run.argtypes = [C.c_int, C.c_int, U, U, U, U, U, V, C.c_int, V, V, V, V, V, V]
    return L


REF_GEOM_FIELDS = ("origin_x", "origin_y", "bwidth", "bheight", "shape", "depth", "nsi", "totns", "sqi_mds", "is_last_quadrant", "has_uv", "bwidth_uv",
                   "bheight_uv")


def reference_geometry(L, sb_size):
    n = 4421 if sb_size == 128 else 1101
    out = np.zeros((n, len(REF_GEOM_FIELDS)), np.int32)
    assert L.drv_md_part_geometry(int(sb_size == 128), out.ctypes.data) == n
    return out


def reference_walk(L, s, k):
    """the reference's own d1 / d2 and EncodePass's walk on superblock k of a scenario -> (walk dict, counters)"""
    n = len(geometry(s.sb_size))
    leaves = np.ascontiguousarray(np.array(s.lists[k], np.uint32).reshape(-1, 3))
    costs = np.array(leaf_costs(s, k), np.uint64)
    fac = np.ascontiguousarray(s.fac, np.int32)
    out_cost, out_state, out_final, counters = np.zeros(n, np.uint64), np.zeros((n, 5), np.uint32), np.zeros(1024, np.uint32), np.zeros(4, np.uint32)
    ox, oy = s.origins[k]
    assert L.drv_md_part_run(int(s.sb_size == 128), int(s.intra), s.w, s.h, ox, oy, s.lams[k], fac.ctypes.data, len(leaves), leaves.ctypes.data,
                             costs.ctypes.data, out_cost.ctypes.data, out_state.ctypes.data, out_final.ctypes.data, counters.ctypes.data) == n
    r = {"cost": out_cost.tolist(), "final": out_final[:int(counters[0])].tolist()}
    for i, key in enumerate(("part", "split", "best", "tested", "mdc")):
        r[key] = out_state[:, i].tolist()
    return r, counters.tolist()
