"""TEST INFRASTRUCTURE: a numpy restatement of mode decision's fast loop as svthip_md_fast_cost_batch_dev and
svthip_md_fast_pick_batch_dev compute it (include/svtav1_hip.h), the constructed cases the CPU and GPU tests share, and the fixture
tests/golden/md_fast.npz (written by tests/golden/make_golden_md_fast.py, which asserts this restatement equal to the reference's own SAD
kernels, RDCOST macro and PreModeDecision; the buffer walk of ProductPerformFastLoop is restated here and pinned by nothing else).

Reference (Source/Lib): Codec/EbProductCodingLoop.c:1282-1459 and :2525-2561, Codec/EbRateDistortionCost.c:764-771 / :1321-1343,
Codec/EbRateDistortionCost.h:215-217, Codec/EbModeDecision.c:393-471."""
import os

import numpy as np

from abi_util import svtav1_hip

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "md_fast.npz")

# the 22 AV1 block sizes, (width, height)
SIZES = ((4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (64, 128),
         (128, 64), (128, 128), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16))

LUMA_GIVEN, SKIP_DISTORTION, INVALID, CHROMA_QUARTER, TYPE_INTER = 1, 2, 4, 8, 16
MAX_CANDIDATES, MAX_BUFFERS = 113, 13
MAX_COST = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_MERGE = 0xFFFFFFFF

# the layouts are the package's, which reads them from include/svtav1_hip.h
DESC_DTYPE, RESULT_DTYPE, GROUP_DTYPE, PICK_DTYPE = (svtav1_hip.md_fast_desc_dtype(), svtav1_hip.md_fast_result_dtype(), svtav1_hip.md_fast_group_dtype(),
                                                     svtav1_hip.md_fast_pick_dtype())


def chroma_size(w, h):
    """blk_geom->bwidth_uv, bheight_uv"""
    return max(4, w // 2), max(4, h // 2)


def round_uv(v):
    """((v >> 3) << 3) / 2: where chroma of a luma position lies (ROUND_UV, round_origin >> 1)"""
    return ((int(v) >> 3) << 3) // 2


def sad(a, b):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).sum())


def rdcost(lambda_, rate, distortion):
    """RDCOST(RM, R, D) = ROUND_POWER_OF_TWO((uint64_t)R * RM, AV1_PROB_COST_SHIFT) + D * (1 << RDDIV_BITS), modulo 2^64"""
    return ((int(rate) * int(lambda_) + 256) >> 9) + (int(distortion) << 7) & 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------------ entry 1

def candidate_sads(src, pred, d, w, h):
    """(SAD Y, SAD Cb, SAD Cr) of one descriptor as plainly measured, flags aside; src and pred are (Y, Cb, Cr) arrays"""
    cw, ch = chroma_size(w, h)
    sx, sy, px, py = int(d["src_x"]), int(d["src_y"]), int(d["pred_x"]), int(d["pred_y"])
    out = [sad(src[0][sy:sy + h, sx:sx + w], pred[0][py:py + h, px:px + w])]
    for k in (1, 2):
        cx, cy, qx, qy = round_uv(sx), round_uv(sy), round_uv(px), round_uv(py)
        out.append(sad(src[k][cy:cy + ch, cx:cx + cw], pred[k][qy:qy + ch, qx:qx + cw]))
    for k, (p, q) in enumerate(((src[0], pred[0]), (src[1], pred[1]), (src[2], pred[2]))):   # the blocks lie inside the planes
        bw, bh = (w, h) if k == 0 else (cw, ch)
        x, y, u, v = (sx, sy, px, py) if k == 0 else (round_uv(sx), round_uv(sy), round_uv(px), round_uv(py))
        assert x + bw <= p.shape[1] and y + bh <= p.shape[0] and u + bw <= q.shape[1] and v + bh <= q.shape[0], (k, d)
    return tuple(out)


def finish(d, sads):
    """(luma, chroma, cost) of a descriptor from its three measured SADs: the flags of :1332-1391 and the cost"""
    flags = int(d["flags"])
    measures = not flags & (SKIP_DISTORTION | INVALID)
    luma = (int(d["luma_given"]) if flags & LUMA_GIVEN else sads[0]) if measures else 0
    chroma = sads[1] + sads[2] if measures and d["has_uv"] else 0
    if flags & CHROMA_QUARTER:
        chroma >>= 2
    cost = int(MAX_COST) if flags & INVALID else rdcost(d["lambda_"], min(int(d["rate"]), int(d["merge_rate"])), luma + chroma)
    return luma, chroma, cost


def fast_cost(src, pred, desc, w, h):
    """svthip_md_fast_cost_batch_dev: RESULT_DTYPE[n]"""
    out = np.zeros(len(desc), RESULT_DTYPE)
    for i, d in enumerate(desc):
        out[i] = finish(d, candidate_sads(src, pred, d, w, h))
    return out


# ------------------------------------------------------------------------------------------------ entry 2

def max_buffers(g):
    return min(int(g["buffer_total_count"]) + 1, int(g["buffer_width"]))


def group_valid(g, n_cand):
    return (1 <= g["count"] <= MAX_CANDIDATES and 1 <= g["buffer_width"] <= MAX_BUFFERS and 1 <= g["buffer_total_count"] <= MAX_BUFFERS - 1
            and int(g["first"]) + int(g["count"]) <= n_cand)


def walk(costs, n_buffers):
    """the buffer replacement of :1284-1459 over candidates with these costs, in walking order -> (cost[13], cand[13]); cand 0xff = empty"""
    cost = [int(MAX_COST)] * MAX_BUFFERS
    cand = [0xFF] * MAX_BUFFERS
    hi = 0
    for k, c in enumerate(costs):
        cost[hi], cand[hi] = int(c), k
        if k + 1 < len(costs):          # if (fastLoopCandidateIndex)
            hi, b = 0, 1
            while True:                 # do { } while (++bufferIndex < bufferIndexEnd)
                highest = cost[hi]
                if highest == int(MAX_COST):
                    break
                if cost[b] > highest:
                    hi = b
                b += 1
                if not b < n_buffers:
                    break
    return cost, cand


def pre_mode_decision(cost, types, total, same):
    """PreModeDecision over buffers with these costs and candidate types (1 INTER_MODE, 2 INTRA_MODE, 0 neither) ->
    (best[], full count, disable_merge_index)"""
    full = max(1, total) if same else max(1, total - 1)
    best = [0]
    if total > 1:
        if same:
            best = list(range(total))
        else:
            highest, worst = cost[0], 0
            for i in range(1, total):
                if cost[i] >= highest:
                    highest, worst = cost[i], i
            best = [i for i in range(total) if i != worst]
    for i in range(full - 1):
        for j in range(i + 1, full):
            if types[best[i]] == 2 and types[best[j]] == 1:
                best[i], best[j] = best[j], best[i]
    return best, full, int(any(types[b] == 1 for b in best[:full]))


def pick_arguments(g, cost, cand, flags):
    """what :2547-2561 hands PreModeDecision for group g after the walk: (types[13], buffer_total_count argument, same_fast_full_candidate)"""
    types = [0 if k == 0xFF else (1 if flags[k] & TYPE_INTER else 2) for k in cand]
    total_count = min(int(g["count"]), int(g["buffer_total_count"]))
    same = int(g["count"]) == total_count
    return types, (total_count if same else max_buffers(g)), same


def pick(result, desc, groups):
    """svthip_md_fast_pick_batch_dev: (PICK_DTYPE[n_groups], number of refused groups)"""
    out = np.zeros(len(groups), PICK_DTYPE)
    out["best"], out["buffer_cand"] = 0xFF, 0xFF
    refused = 0
    for i, g in enumerate(groups):
        if not group_valid(g, len(result)):
            refused += 1
            continue
        rows = slice(int(g["first"]), int(g["first"]) + int(g["count"]))
        cost, cand = walk(result["cost"][rows], max_buffers(g))
        types, total, same = pick_arguments(g, cost, cand, desc["flags"][rows])
        best, full, dmi = pre_mode_decision(cost, types, total, same)
        out[i]["best"][:len(best)] = best
        out[i]["buffer_cand"] = cand
        out[i]["full_count"], out[i]["disable_merge_index"] = full, dmi
    return out, refused


# ------------------------------------------------------------------------------------------------ constructed cases

SRC_W, SRC_H = 200, 160     # the source picture of every case
N_TILES = 6                 # prediction tiles per case: a 3 x 2 grid in the pool planes


def _texture(w, h, seed):
    """a plane of bytes that looks random and is the same everywhere: no generator state involved"""
    y, x = np.mgrid[0:h, 0:w].astype(np.uint64)
    v = (x * np.uint64(2654435761) + y * np.uint64(40503) + np.uint64(seed) * np.uint64(7919) + (x * y >> np.uint64(2)) * np.uint64(2246822519))
    v ^= v >> np.uint64(13)
    v = v * np.uint64(3266489917) & np.uint64(0xFFFFFFFF)
    return ((v >> np.uint64(11)) & np.uint64(255)).astype(np.uint8)


def source_planes():
    """(Y, Cb, Cr) of the 200 x 160 source picture; the extremes occur"""
    y = _texture(SRC_W, SRC_H, 1)
    y[::7, ::5] = 255
    y[3::11, 2::3] = 0
    return y, _texture(SRC_W // 2, SRC_H // 2, 2), _texture(SRC_W // 2, SRC_H // 2, 3)


def tile_origins(w, h):
    """luma positions of the six tiles in the pool planes, multiples of 8 with room for a ring of samples around each luma and chroma tile, and
    the pool's (width, height)"""
    pw, ph = (w + 15) // 8 * 8, (h + 15) // 8 * 8
    origins = [(8 + (t % 3) * pw, 8 + (t // 3) * ph) for t in range(N_TILES)]
    return origins, (8 + 3 * pw, 8 + 2 * ph)


def pool_planes(size_index, src):
    """(Y, Cb, Cr) pool planes of one size: tile t is the source block that candidate t is compared with, disturbed more and more with t (never left equal),
    and the samples right around every luma and chroma tile are 0 and 255 in turn, so a sum that strays outside a tile changes"""
    w, h = SIZES[size_index]
    cw, ch = chroma_size(w, h)
    origins, (pool_w, pool_h) = tile_origins(w, h)
    planes = [_texture(pool_w, pool_h, 10 + size_index), _texture(pool_w // 2, pool_h // 2, 40 + size_index),
              _texture(pool_w // 2, pool_h // 2, 70 + size_index)]
    for t, (px, py) in enumerate(origins):
        sx, sy = source_position(size_index, t)
        for k in range(3):
            bw, bh = (w, h) if k == 0 else (cw, ch)
            x, y, u, v = (px, py, sx, sy) if k == 0 else (round_uv(px), round_uv(py), round_uv(sx), round_uv(sy))
            noise = _texture(bw, bh, 100 + 3 * t + k).astype(np.int32) - 128
            block = src[k][v:v + bh, u:u + bw].astype(np.int32) + noise * (t + 1) // 8
            ring = planes[k][y - 1:y + bh + 1, x - 1:x + bw + 1]
            ring[...] = np.where((np.add.outer(np.arange(bh + 2), np.arange(bw + 2)) + t) & 1, 255, 0)
            planes[k][y:y + bh, x:x + bw] = np.clip(block, 0, 255)
    return tuple(planes)


def source_position(size_index, t):
    """where candidate t of a size reads the source: multiples of 4 that are mostly no multiples of 8, the last block in the picture's
    last rows and columns"""
    w, h = SIZES[size_index]
    room_x, room_y = SRC_W - w, SRC_H - h
    if t % N_TILES == N_TILES - 1:
        return room_x, room_y
    return (4 * (3 * t + size_index)) % (room_x + 4) // 4 * 4, (4 * (5 * t + 2 * size_index)) % (room_y + 4) // 4 * 4


def flag_sets():
    """every flag alone, none, and combinations (TYPE_INTER is carried along for the pick)"""
    return (0, LUMA_GIVEN, SKIP_DISTORTION, INVALID, CHROMA_QUARTER, TYPE_INTER, LUMA_GIVEN | CHROMA_QUARTER, LUMA_GIVEN | SKIP_DISTORTION,
            INVALID | CHROMA_QUARTER | TYPE_INTER, SKIP_DISTORTION | CHROMA_QUARTER, LUMA_GIVEN | INVALID, CHROMA_QUARTER | TYPE_INTER,
            LUMA_GIVEN | SKIP_DISTORTION | INVALID | CHROMA_QUARTER | TYPE_INTER)


def descriptors(size_index, n, variant=0):
    """n descriptors of one size over the six tiles: has_uv both ways, every flag set of flag_sets(), merge rates below and above the rate"""
    w, h = SIZES[size_index]
    origins, _ = tile_origins(w, h)
    sets = flag_sets()
    d = np.zeros(n, DESC_DTYPE)
    for i in range(n):
        t = i % N_TILES
        # the last tile is always compared with the source picture's last block; the others wander with i and the variant
        d[i]["src_x"], d[i]["src_y"] = source_position(size_index, t if t == N_TILES - 1 else (i + variant) % (2 * N_TILES))
        d[i]["pred_x"], d[i]["pred_y"] = origins[t]
        d[i]["rate"] = 1000 + 977 * i + 31 * size_index
        d[i]["merge_rate"] = NO_MERGE if i % 3 else 600 + 1500 * (i % 2) + 13 * i
        d[i]["lambda_"] = (97 + 211 * i + variant) if i % 5 else 0xFFFFFFF1
        d[i]["luma_given"] = 12345 + 7 * i
        d[i]["has_uv"] = 0 if (i + variant) % 4 == 3 else 1
        d[i]["flags"] = sets[(i + variant) % len(sets)] if n > 1 else 0
        d[i]["reserved"] = 0xA5     # ignored
    return d


# the pick: (name, costs in walking order, types (1 inter / 2 intra) in walking order, buffer_total_count, buffer_width)
def pick_cases():
    M = int(MAX_COST)
    cases = [
        ("one candidate", [700], [2], 1, 13),
        ("one candidate, inter", [700], [1], 3, 5),
        ("count == buffer_total_count", [50, 40, 60, 30], [2, 1, 2, 1], 4, 13),
        ("count < buffer_total_count", [50, 40, 60], [2, 2, 1], 7, 13),
        ("count > maxBuffers", [50, 40, 60, 30, 70, 20, 80, 10, 45], [2, 1, 2, 1, 2, 2, 1, 1, 2], 3, 13),
        ("count > maxBuffers, width binds", [50, 40, 60, 30, 70, 20, 80, 10, 45], [1, 2, 1, 2, 1, 1, 2, 2, 1], 9, 5),
        # the walk's strict >: of two equal highest costs the FIRST buffer stays the one to replace
        ("walk tie, first of equals is replaced", [90, 90, 10, 20, 5], [2, 1, 2, 1, 2], 2, 13),
        ("walk tie among three", [90, 30, 90, 90, 10, 95, 7], [1, 2, 2, 1, 2, 1, 2], 3, 13),
        # PreModeDecision's >=: of two equal highest costs the LAST buffer is left out
        ("pre-mode-decision tie, last of equals is left out", [80, 10, 80, 5], [2, 1, 1, 2], 2, 13),
        ("pre-mode-decision tie on every buffer", [33, 33, 33, 33, 33, 33], [2, 1, 2, 1, 2, 1], 3, 13),
        ("every cost ~0", [M, M, M, M, M], [2, 1, 2, 1, 1], 3, 13),
        ("every cost ~0, count == buffer_total_count", [M, M, M], [1, 2, 1], 3, 13),
        ("a cost of ~0 in the middle", [50, M, 40, 30, 60, 20], [2, 1, 2, 1, 2, 1], 3, 13),
        ("a cost of ~0 first", [M, 40, 30, 60], [1, 2, 1, 2], 6, 13),
        ("intra and inter interleaved", [10, 20, 30, 40, 50, 60, 70, 80], [2, 1, 2, 1, 2, 1, 2, 1], 8, 13),
        ("intra before inter, one left out", [10, 20, 30, 40, 50, 60, 70, 80, 90, 5], [2, 2, 2, 1, 1, 2, 1, 2, 1, 1], 6, 13),
        ("all intra", [10, 20, 30, 40, 50], [2, 2, 2, 2, 2], 3, 13),
        ("buffer_width 1", [50, 40, 60], [2, 1, 2], 2, 1),
        ("buffer_width 2", [50, 40, 60, 30], [2, 1, 2, 1], 5, 2),
    ]
    costs = [int(v) for v in (_texture(MAX_CANDIDATES, 1, 9)[0].astype(np.int64) * 1000003 % 99991)]
    types = [1 + int(v & 1) for v in _texture(MAX_CANDIDATES, 1, 8)[0]]
    cases.append(("113 candidates, 13 buffers", costs, types, 12, 13))
    costs2 = list(costs)
    costs2[5::9] = [costs2[4]] * len(costs2[5::9])   # runs of equal costs
    cases.append(("113 candidates with equal costs, 13 buffers", costs2, types[::-1], 12, 13))
    cases.append(("113 candidates, 5 buffers", costs[::-1], types, 4, 5))
    return cases


def pick_inputs(cases=None):
    """the cases as the arrays the entry takes: (RESULT_DTYPE[n], DESC_DTYPE[n], GROUP_DTYPE[n_groups])"""
    cases = pick_cases() if cases is None else cases
    n = sum(len(c[1]) for c in cases)
    result, desc, groups = np.zeros(n, RESULT_DTYPE), np.zeros(n, DESC_DTYPE), np.zeros(len(cases), GROUP_DTYPE)
    at = 0
    for i, (_, costs, types, total, width) in enumerate(cases):
        rows = slice(at, at + len(costs))
        result["cost"][rows] = np.array(costs, np.uint64)
        desc["flags"][rows] = [TYPE_INTER if t == 1 else 0 for t in types]
        groups[i] = (at, len(costs), total, width)
        at += len(costs)
    return result, desc, groups


_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(FIXTURE) as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE
