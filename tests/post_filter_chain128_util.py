"""The front of the post-reconstruction filter chain on pictures coded with 128-wide blocks, as one run of the restatements, for
tests/test_post_filter_chain128_vs_ref.py and tests/test_post_filter_chain128_gpu.py.  TEST INFRASTRUCTURE: numpy only.

  deblocking level pick -> deblocking -> CDEF search and pick for 128-wide blocks -> CDEF frame filter

Two 328 x 200 pictures (8 and 10 bits) with the block layout of case B of tests/cdef128_util.py: BLOCK_128X128 full and clipped,
BLOCK_128X64, BLOCK_64X128, small blocks in between; the wide blocks carry TX_64X64 (their chroma transform, 32x32, follows from the
block size), the small ones their own size.  The deblocking restatement and kernels meet 128-wide sb_types here for the first time.  The
pictures are regenerated from their seeds; tests/golden/post_filter_chain128.npz holds digests of the inputs and what the reference's
own stages made of them as a chain (tests/golden/make_golden_post_filter_chain128.py)."""
import os

import numpy as np

import cdef128_util as c128
import cdef_util as cu
import dlf_util as du
import post_filter_chain_util as pc

FIXTURE = os.path.join(pc.ROOT, "tests", "golden", "post_filter_chain128.npz")
W, H = 328, 200
PICTURES = {"A": {"seed": 11, "bd": 8, "last_levels": (20, 20, 20, 20), "base_qindex": 100},
            "B": {"seed": 12, "bd": 10, "last_levels": (20, 20, 20, 20), "base_qindex": 160}}
PARAM_KEYS = ("seed", "bd", "base_qindex")
PLANE_STAGES = ("dbk", "cdef")
SMALL = (("levels", np.int32), ("masks", np.uint64), ("mse", np.uint64), ("counted", np.uint8), ("cdef_result", np.int32), ("fb_strength", np.int8))
ORDER = ("levels", "masks", "dbk", "mse", "counted", "cdef_result", "fb_strength", "cdef")
TX_OF_BLOCK = {c128.BLOCK_8X8: du.TX_OF[(8, 8)], c128.BLOCK_16X16: du.TX_OF[(16, 16)], c128.BLOCK_64X128: du.TX_OF[(64, 64)],
               c128.BLOCK_128X64: du.TX_OF[(64, 64)], c128.BLOCK_128X128: du.TX_OF[(64, 64)]}


def make_picture(name):
    """(mi, recon planes, source planes): the grid covers whole 64x64 superblocks (64 rows of 96 cells), as the deblocking entries take it"""
    P = PICTURES[name]
    rng = np.random.default_rng(P["seed"])
    mi = np.zeros(((H + 63) // 64 * 16, (W + 63) // 64 * 16), du.LF_MI_DTYPE)
    mi["sb_type"], mi["tx_size"], mi["flags"] = c128.BLOCK_16X16, TX_OF_BLOCK[c128.BLOCK_16X16], 1
    sb = c128.make_grid("B", W, H)
    mi["sb_type"][:H // 4, :W // 4] = sb
    for t, tx in TX_OF_BLOCK.items():
        mi["tx_size"][:H // 4, :W // 4][sb == t] = tx
    mi["flags"][:H // 4, :W // 4] = c128.make_skip(rng, "B", W, H)
    recon, source = du.random_picture(rng, W, H, P["bd"], mi)
    return mi, recon, source


def grids(mi):
    """the skip map and the sb_type map of the picture, one byte per 4x4 luma cell"""
    return (np.ascontiguousarray((mi["flags"] & 1)[:H // 4, :W // 4].astype(np.uint8)), np.ascontiguousarray(mi["sb_type"][:H // 4, :W // 4]))


def run_chain(recon, source, mi, bd, last_levels, base_qindex):
    out = {}
    levels, masks, _ = du.pick_filter_level(recon, source, mi, last_levels, 0, 0, bd)
    out["levels"], out["masks"] = np.array(levels, np.int32), np.array(masks, np.uint64)
    dbk = [p.copy() for p in recon]
    du.loop_filter_frame(dbk, mi, levels, 0, 0, 3, bd)
    out["dbk"] = dbk
    skip, sb = grids(mi)
    mse, counted = c128.search(dbk, source, skip, sb, W, H, bd, base_qindex)
    res, fbs = c128.pick(mse, counted, sb, W, H, base_qindex, bd)
    out["mse"], out["counted"], out["cdef_result"], out["fb_strength"] = mse, counted, res.reshape(1).view(np.int32).copy(), fbs
    out["cdef"] = c128.frame(dbk, skip, W, H, bd, res, fbs)
    return out


def chain_of(name):
    P = PICTURES[name]
    mi, recon, source = make_picture(name)
    return mi, recon, source, run_chain(recon, source, mi, P["bd"], P["last_levels"], P["base_qindex"])


def conditions(recon, chain):
    res = chain["cdef_result"].view(cu.RESULT_DTYPE)[0]
    fbs = chain["fb_strength"]
    return {"all four levels are not 0": all(int(v) for v in chain["levels"]), "cdef_bits > 0": int(res["cdef_bits"]) > 0,
            "fewer fbs are counted than carry an index": int(chain["counted"].sum()) < int((fbs >= 0).sum()),
            "a wide fb is left out with its twin": bool(fbs[14] == -1 and fbs[15] == -1),
            "deblocking changes every plane": all(not np.array_equal(a, b) for a, b in zip(chain["dbk"], recon)),
            "CDEF changes every plane": all(not np.array_equal(a, b) for a, b in zip(chain["cdef"], chain["dbk"]))}


_FIXTURE = {}


def fixture():
    if not _FIXTURE:
        _FIXTURE.update(np.load(FIXTURE))
    return _FIXTURE


def expected(name, recon=None):
    """the SMALL arrays, sha256 of the inputs, `digest_<stage>` and, with `recon`, the planes (stored as differences against the stage before)"""
    z = fixture()
    out = {k: z[f"{name}_{k}"] for k, _ in SMALL}
    for k in ("recon", "source", "mi"):
        out["sha256_" + k] = z[f"{name}_sha256_{k}"]
    prev = recon
    for k in PLANE_STAGES:
        out["digest_" + k] = z[f"{name}_digest_{k}"]
        if prev is not None:
            prev = out[k] = [(prev[p].astype(np.int32) + z[f"{name}_{k}_d{p}"]).astype(prev[p].dtype) for p in range(3)]
    return out


def first_difference(got, want, only=None):
    """the first stage, in chain order, at which `got` is not `want`: a string naming it, or None"""
    for k in ORDER:
        if only is not None and k not in only:
            continue
        if k in PLANE_STAGES:
            for p in range(3):
                if not np.array_equal(got[k][p], want[k][p]):
                    at = np.argwhere(got[k][p] != want[k][p])
                    return f"{k}, plane {p}: {len(at)} samples differ, the first at (row, column) {at[0].tolist()}"
        else:
            g, w_ = np.asarray(got[k]).reshape(-1), np.asarray(want[k]).reshape(-1)
            if g.shape != w_.shape or not np.array_equal(g.astype(w_.dtype), w_):
                return f"{k}: differs" + ("" if g.shape != w_.shape else f" at {np.flatnonzero(g.astype(w_.dtype) != w_)[:6].tolist()}")
    return None
