"""GPU: the full loop and the partition decision as one chain on device-made hand-overs, for one 64x64 superblock.
svthip_md_full_loop_batch_dev runs for the 32x32, 32x16, 16x32 and 16x16 blocks of the superblock (scenarios built with the helpers of
tests/md_full_util.py), each call into its own sub-range of ONE decision array and its own band of ONE tile pool (the `recon` of the full
loop); svthip_md_partition_picture_dev then reads those device-made costs and tiles: neither crosses the host.  Between the two the test
reads the context's refusal counter (the full loop counts slots whose TxType has no network), so that what the partition adds to it, which
must be nothing, can be asserted.  The final picture must equal the restatement's composition (tests/md_part_util.py) of the restatement's
tiles (md_full_util.full_loop)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import md_full_util as fu  # noqa: E402
import md_part_util as pu  # noqa: E402
import svtav1_hip  # noqa: E402
from test_md_full_gpu import GUARD, _Call as _FullCall, _dev, _Planes  # noqa: E402

pytestmark = pytest.mark.gpu

POOL_SHAPES = [(256, 64), (128, 32), (128, 32)]
# size -> (shape of the md scan, where group g's winner tile goes in the pool)
SIZES = {(32, 32): (0, lambda g: ((g % 2) * 32, (g // 2) * 32)), (32, 16): (1, lambda g: ((g % 2) * 32, 64 + (g // 2) * 16)),
         (16, 32): (2, lambda g: ((g % 4) * 16, 128 + (g // 4) * 32)), (16, 16): (0, lambda g: ((g % 4) * 16, 192 + (g // 4) * 16))}


def _full_scenario(w, h, n_groups):
    """a scenario of md_full_util for n_groups blocks of w x h whose winners land at the pool positions above"""
    name = f"part_chain_{w}x{h}"
    fu.CASES[name] = ((w, h), n_groups, 2, "none", 0)
    try:
        s = fu.scenario(name)
    finally:
        del fu.CASES[name]
    for g in range(n_groups):
        rows = slice(int(s.groups[g]["first"]), int(s.groups[g]["first"]) + int(s.groups[g]["count"]))
        s.full["recon_x"][rows], s.full["recon_y"][rows] = SIZES[(w, h)][1](g)
    s.recon_shape = POOL_SHAPES
    return s


def test_full_loop_costs_and_tiles_become_a_partitioned_picture(hip_ctx):
    torch = pytest.importorskip("torch")
    from oracle.binding import Oracle
    geom = pu.geometry(64)
    squares32 = [25 + q * 269 for q in range(4)]
    squares16 = [sq + 25 + k * 61 for sq in squares32 for k in range(4)]
    # the leaves in md-scan order: per 32x32 its N, H and V blocks (5 d1 blocks), then its four 16x16 (split_flag 0: the fourth climbs)
    blocks = {(32, 32): squares32, (32, 16): [sq + 1 + i for sq in squares32 for i in range(2)], (16, 32): [sq + 3 + i for sq in squares32 for i in range(2)],
              (16, 16): squares16}
    scen = {wh: _full_scenario(*wh, len(m)) for wh, m in blocks.items()}
    base, at = {}, 0
    for wh in blocks:
        base[wh], at = at, at + len(blocks[wh])
    n_decision = at
    where = {m: (wh, g) for wh, ms in blocks.items() for g, m in enumerate(ms)}
    order = sorted(where)
    leaves = np.zeros(len(order), pu.LEAF_DTYPE)
    for i, m in enumerate(order):
        wh, g = where[m]
        px, py = SIZES[wh][1](g)
        leaves[i] = (base[wh] + g, m, 1 if wh == (16, 16) else 5, int(wh != (16, 16)), px, py, 0)
        assert (int(geom["bwidth"][m]), int(geom["bheight"][m]), int(geom["shape"][m])) == (*wh, SIZES[wh][0])
    sbs = np.zeros(1, pu.SB_DTYPE)
    sbs[0] = (0, len(leaves), 777, 0, 0)
    fac = np.random.default_rng(5).integers(150, 3000, (20, 11)).astype(np.int32)

    # the restatement: the full loop per size, its decisions and its tiles; then the walk and the composition
    want_pool = [np.full(sh, fu.RECON_FILL, np.uint8) for sh in POOL_SHAPES]
    want_cost = np.zeros(n_decision, np.uint64)
    oracle, st_refused = Oracle(), []
    for wh, s in scen.items():
        st = fu.full_loop(oracle, s)
        st_refused.append(st["refused"])
        want_cost[base[wh]:base[wh] + s.n_groups] = st["decision"]["cost"]
        y0 = {(32, 32): 0, (32, 16): 64, (16, 32): 128, (16, 16): 192}[wh]
        for p in range(3):
            a, b = (y0, y0 + 64) if p == 0 else (y0 // 2, y0 // 2 + 32)
            want_pool[p][a:b] = st["recon"][p][a:b]
    r = pu.walk(64, [(int(x["mds_idx"]), int(x["tot_d1_blocks"]), int(x["split_flag"])) for x in leaves], [int(want_cost[x["decision_index"]]) for x in leaves],
                777, fac, False)
    assert r["part"][0] == pu.SPLIT and len(r["final"]) >= 4
    want = [np.full((64, 64), 0xA5, np.uint8), np.full((32, 32), 0xA5, np.uint8), np.full((32, 32), 0xA5, np.uint8)]
    leaf_of = {m: i for i, m in enumerate(order)}
    for m in r["final"]:
        f = np.zeros((), pu.FINAL_DTYPE)
        f["x"], f["y"], f["bwidth"], f["bheight"], f["has_uv"] = geom["origin_x"][m], geom["origin_y"][m], geom["bwidth"][m], geom["bheight"][m], geom["has_uv"][m]
        pu.compose_block(want, want_pool, f, leaves[leaf_of[m]])

    # the device: four full-loop calls into one decision array and one pool, then the partition and the composition
    hip_ctx.inter_pred_refused()
    pool = _Planes(torch, [np.full(sh, fu.RECON_FILL, np.uint8) for sh in POOL_SHAPES], 0)
    dst = _Planes(torch, [np.full(p.shape, 0xA5, np.uint8) for p in want], 0)
    d_decision = torch.full(((n_decision + 1) * 16,), GUARD, dtype=torch.uint8, device="cuda:0")
    calls = [_FullCall(torch, hip_ctx, s, 0) for s in scen.values()]
    d_sb, d_leaf = _dev(torch, sbs), _dev(torch, leaves)
    d_result = torch.zeros(1101 * 16, dtype=torch.uint8, device="cuda:0")
    d_final = torch.zeros(256 * 16, dtype=torch.uint8, device="cuda:0")
    d_count = torch.zeros(4, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()   # torch's fills above are not ordered before the library's stream; the chain itself has no synchronisation
    for call, (wh, s) in zip(calls, scen.items()):
        args = call.args(fu.LUMA | fu.CHROMA | fu.DECIDE)
        args["recon"], args["d_decision"] = pool.arg, d_decision.data_ptr() + base[wh] * 16
        hip_ctx.md_full_loop_batch_dev(**args)
    full_loop_refused = sum(st_refused)
    if full_loop_refused:
        with pytest.raises(svtav1_hip.SvtHipError, match=rf"80001005: {full_loop_refused} PU\(s\) or unit\(s\) refused"):
            hip_ctx.inter_pred_refused()
    assert hip_ctx.inter_pred_refused() == 0
    hip_ctx.md_partition_picture_dev(d_sb.data_ptr(), 1, d_leaf.data_ptr(), len(leaves), d_decision.data_ptr(), n_decision, 64, 0, fac, d_result.data_ptr(),
                                     d_final.data_ptr(), d_count.data_ptr(), pool.arg, 64, 256, dst.arg, 64, 64)
    hip_ctx.synchronize()
    torch.cuda.synchronize()
    assert sum(s.pick_refused for s in scen.values()) == 0
    assert hip_ctx.inter_pred_refused() == 0   # every final block has a leaf and a tile inside the planes: the partition counted nothing
    raw = d_decision.cpu().numpy()
    assert (raw[-16:] == GUARD).all()
    assert np.array_equal(raw[:-16].view(pu.DECISION_DTYPE)["cost"], want_cost)
    assert all(np.array_equal(a, b) for a, b in zip(pool.download(), want_pool)), "the tile pool is not the restatement's"
    result = d_result.cpu().numpy().view(pu.RESULT_DTYPE)
    assert np.array_equal(result["cost"], np.array(r["cost"], np.uint64)) and result["part"].tolist() == r["part"]
    count = int(d_count.cpu().numpy().view(np.uint32)[0])
    assert d_final.cpu().numpy().view(pu.FINAL_DTYPE)["mds_idx"][:count].tolist() == r["final"]
    got = dst.download()
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), "the composed picture is not the restatement's"
    assert not (got[0] == 0xA5).all(axis=None)
