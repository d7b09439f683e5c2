"""Writes tests/golden/md_chain.npz from the reference's own mode-decision stages run on the chain's data (tests/md_chain_util.py): at every
stage the reference driver that already exists for that stage is fed what the chain holds there -- the PU descriptors and pictures
(ref_interp_search_driver.c), the descriptors with the searched filters (ref_inter_pred_driver.c), the neighbour picture's edges
(ref_intra_pred_driver.c), the predicted pool (ref_md_fast_driver.c), the luma the LUMA stage reconstructed and the pool's DC tiles
(ref_cfl_driver.c), the levels of the 66 candidate tiles a block (ref_coeff_rate_driver.c), the distortions, rates and costs of the slots
(the leaves and the decision loop of ref_md_full_driver.c) -- and what the reference returned is asserted equal to the restated chain's stage
and stored.  The drivers and the calls are those of make_golden_md_ifs.py, make_golden_inter_pred.py, make_golden_intra_pred.py,
make_golden_md_fast.py, make_golden_cfl.py, rate_util.py and md_full_util.py; this file holds no reference text.  The T/Q chain itself stays
pinned through the oracle (test_tq_vs_ref.py), and the walk of the fast loop's buffers and the slot bookkeeping of the full loop through
their restatements, as in the fixtures of the single stages; so do the PAETH blocks, for which the reference has no predictor.  Run in
the build container only, where the reference exists: the fixture is data.

    python tests/golden/make_golden_md_chain.py

Contents, per size n of md_chain_util.SIZES (the inputs are regenerated from their seeds, not stored)
  {n}_sha256_src, _refs, _nb, _desc      sha256 of the generated pictures and descriptor arrays
  {n}_ifs, {n}_pu                        the search's result rows; the PU descriptors after the write-back       (rows of bytes)
  {n}_fast, {n}_picks                    the fast loop's result rows and picks
  {n}_cfl                                the alpha decisions of the slots the CfL service applies to
  {n}_result, {n}_decision               the full loop's result rows and decisions
  {n}_digest_pool_luma, _slot_luma, _pool_chroma, _recon   sha256 of the plane sets after their stage
  {n}_refused                            the refusals the chain counts
  {n}_measures                           md_chain_util.MEASURES: the figures behind the conditions on the inputs"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import cfl_util as cu  # noqa: E402
import inter_pred_util as ipu  # noqa: E402
import intra_pred_util as iu  # noqa: E402
import make_golden_cfl as mg_cfl  # noqa: E402
import make_golden_inter_pred as mg_ip  # noqa: E402
import make_golden_intra_pred as mg_intra  # noqa: E402
import make_golden_md_fast as mg_fast  # noqa: E402
import make_golden_md_ifs as mg_ifs  # noqa: E402
import md_chain_util as mc  # noqa: E402
import md_fast_util as mu  # noqa: E402
import md_full_util as fu  # noqa: E402
import md_ifs_util as su  # noqa: E402
import rate_util  # noqa: E402
from make_golden_cdef import save  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


class Drivers:
    """the seven reference drivers, each built in a directory of its own under `tmp`"""

    def __init__(self, tmp):
        def sub(name):
            d = os.path.join(tmp, name)
            os.makedirs(d)
            return d
        self.ifs, self.ip, self.intra = mg_ifs.build_driver(sub("ifs")), mg_ip.build_driver(sub("ip")), mg_intra.build_driver(sub("intra"))
        self.fast, self.cfl, self.full = mg_fast.build_driver(sub("fast")), mg_cfl.build_driver(sub("cfl")), fu.build_reference_driver(sub("full"))
        self.rate = rate_util.build_reference_driver(sub("rate"))
        z = np.load(os.path.join(ROOT, "tests", "golden", "coeff_rate.npz"))
        assert self.rate.drv_init(int(z["qindices"][1])) == 0          # the tables md_full_util.shared() takes from coeff_rate.npz


def _intra_reference(L, s, plane, pool, restated):
    """the reference's blocks of the intra candidates of `plane`, from edges gathered out of the neighbour picture into the driver's layout;
    the reference has no PAETH predictor (tests/intra_pred_util.py: random_case), those blocks are the restatement's"""
    edge, base = mc._flat_with_row_above(s.nb[plane])
    d, ts = mc.intra_descs(s, plane, s.nb[plane].shape[1], base, pool.shape[1], 0)
    txw, txh = iu.TX_SIZES_WH[ts]
    per = 4 + 2 * txw + 2 * txh
    packed, d2 = np.zeros(len(d) * per, np.uint8), d.copy()
    for i, e in enumerate(d):
        ao, lo, ls = int(e["above_offset"]), int(e["left_offset"]), int(e["left_stride"])
        packed[i * per + 3:i * per + 4 + 2 * txw] = edge[np.clip(ao - 1 + np.arange(2 * txw + 1), 0, len(edge) - 1)]
        packed[i * per + 4 + 2 * txw:(i + 1) * per] = edge[np.clip(lo + np.arange(2 * txh) * ls, 0, len(edge) - 1)]
        d2[i]["above_offset"], d2[i]["left_offset"], d2[i]["left_stride"] = i * per + 4, i * per + 4 + 2 * txw, 1
    has = d["mode"] != iu.PAETH
    blocks = np.zeros((len(d), txh, txw), np.uint8)
    blocks[has] = mg_intra.reference_blocks(L, packed, d2[has], ts, 8)
    for e, b, ref in zip(d, blocks, has):
        y, x = divmod(int(e["dst_offset"]), pool.shape[1])
        pool[y:y + txh, x:x + txw] = b if ref else restated[y:y + txh, x:x + txw]


def _leaf_tuples(s, chain, slots, post):
    """md_full_util.leaf_tuples' arrays for the slots: the distortions, rates and bits as the leaves take them (`post`: after Av1TuCalcCostLuma)"""
    st, res = chain["state"], chain["result"]
    t = {k: [] for k in ("lam", "bits", "y", "cb", "cr", "luma_rate", "chroma_rate", "skip_rate", "inter", "merge", "has_uv", "eob", "zero_bits", "skip_ctx",
                         "txb_ctx", "tx_size")}
    shift = rate_util.tx_scale_shift(s.ts_y)
    for k in slots:
        row = st["slots"][k]["row"]
        f, d, lu, r = s.fast[row], chain["full"][row], st["luma"][k], res[k]
        raw = [(v + lu["energy"]) >> shift if shift >= 0 else (v + lu["energy"]) << -shift for v in lu["dist"]]
        merge = int(d["skip_mode_rate"]) != fu.NONE
        for name, v in (("lam", d["lambda_"]), ("bits", r["coeff_bits"] if post else [lu["bits"], r["coeff_bits"][1], r["coeff_bits"][2]]),
                        ("y", r["y_distortion"] if post else raw), ("cb", r["cb_distortion"]), ("cr", r["cr_distortion"]), ("luma_rate", d["luma_rate"]),
                        ("chroma_rate", d["chroma_rate"]), ("skip_rate", d["skip_mode_rate"] if merge else 0), ("inter", bool(f["flags"] & mu.TYPE_INTER)),
                        ("merge", merge), ("has_uv", f["has_uv"]), ("eob", r["eob"]), ("zero_bits", 0), ("skip_ctx", 0), ("txb_ctx", min(int(d["txb_skip_ctx"][0]), 12)),
                        ("tx_size", s.ts_y)):
            t[name].append(np.asarray(v, np.uint64))
    return {k: np.array(v, np.uint64) for k, v in t.items()}


def reference_chain(D, name, oracle):
    """the reference's stages on the data of the restated chain of size `name` (md_chain_util.chain_of with `oracle`), by the names of
    md_chain_util.STAGES; every stage is asserted equal to the restated chain's as soon as it is there, so the first restatement that differs
    is the one named"""
    s0 = mc.make_scenario(name)
    s, mine = mc.chain_of(name, oracle)
    w, h, cw, ch = s.w, s.h, s.cw, s.ch
    out = {}

    def stage(*keys):
        diff = mc.first_difference(mine, out, only=keys)
        assert diff is None, f"size {name}: the restated chain differs from the reference's stages at {diff}"

    # 1. interpolation_filter_search on the searched prefix, its filters into the descriptors
    out["ifs"] = np.zeros(s.n_search, su.IFS_RESULT_DTYPE)
    for i in range(s.n_search):
        out["ifs"][i] = mg_ifs.reference_search(D.ifs, (s.ref0, s.ref1, tuple(s.src)), s0.pu[i], s0.ifs_desc[i], w, h, mc.QUANTIZER, 1 if s.ifs == "fast" else 2, 1)
    out["pu"] = s0.pu.copy()
    out["pu"]["interp_filters"][:s.n_search] = out["ifs"]["interp_filters"]
    stage("ifs", "pu")
    # 2. av1_inter_prediction of every PU the device does not refuse, 3. the intra predictors, into the pool
    pool = ipu.Picture(*(p.copy() for p in s0.pool), 0)
    keep = np.array([i for i, d in enumerate(out["pu"]) if not (d["pred_direction"] == 2 and ipu.sub8x8(d, w, h))])
    rft = np.array([(mg_ip.LAST, mg_ip.BWDREF, 8)[int(d["pred_direction"])] for d in out["pu"]], np.int32)
    assert all(D.ip.drv_own_list(int(r)) == int(d["own_list"]) for r, d in zip(rft, out["pu"]) if d["pred_direction"] != 2)
    mg_ip.reference_predict(D.ip, (s.ref0, s.ref1), pool, out["pu"][keep], rft[keep], w, h, 8)
    for p, plane in enumerate((pool.y, pool.cb, pool.cr)):
        _intra_reference(D.intra, s0, p, plane, (mine["pool_luma"] + mine["pool_chroma_dc"])[p])
    out["pool_luma"] = [pool.y]
    stage("pool_luma")
    assert np.array_equal(pool.cb, mine["pool_chroma_dc"][0]) and np.array_equal(pool.cr, mine["pool_chroma_dc"][1]), f"size {name}: the pool's chroma before CfL differs"
    # 4. the SAD kernels and RDCOST, 5. PreModeDecision on the walked buffers
    planes = [pool.y, pool.cb, pool.cr]
    out["fast"] = np.zeros(s.n_cand, mu.RESULT_DTYPE)
    for i, d in enumerate(s.fast):
        out["fast"][i] = mg_fast.reference_result(D.fast, d, mg_fast.reference_sads(D.fast, s.src, planes, d, w, h))
    out["picks"] = mine["picks"].copy()
    for g, grp in enumerate(s.groups):
        if mu.group_valid(grp, s.n_cand):
            rows = slice(int(grp["first"]), int(grp["first"]) + int(grp["count"]))
            cost, cand = mu.walk(out["fast"]["cost"][rows], mu.max_buffers(grp))
            out["picks"][g] = mg_fast.reference_pick(D.fast, grp, cost, cand, s.fast["flags"][rows])
    stage("fast", "picks")
    # 7. the CfL service: cfl_luma_subsampling, subtract_average and cfl_predict for the 66 tiles, Av1TuEstimateCoeffBits, cfl_rd_pick_alpha
    st = mine["state"]
    out["slot_luma"] = mine["slot_luma"]                           # the T/Q chain: the oracle's (test_tq_vs_ref.py)
    out["cfl"], out["pool_chroma"] = np.zeros(len(mine["cfl"]), cu.DECISION), [pool.cb, pool.cr]
    if len(mine["cfl"]):
        luma, desc, npx = st["slot"][0].reshape(-1), mine["cfl_desc"], cw * ch
        at = np.arange(ch)[:, None] * int(desc[0]["chroma_stride"]) + np.arange(cw)[None, :]
        for a in range(-16, 17):
            if a:
                d = desc.copy()
                d["alpha_idx"], d["alpha_signs"] = cu.alpha_to_fields(a, a)
                cb, cr, _ = mg_cfl.reference_predict(D.cfl, luma, pool.cb.reshape(-1), pool.cr.reshape(-1), d, w, h, 8)
            else:
                cb, cr = pool.cb.reshape(-1), pool.cr.reshape(-1)
            for i, e in enumerate(desc):
                assert np.array_equal(cb[int(e["cb_offset"]) + at].reshape(-1), mine["cfl_cand"][i, 0, a + 16]), (name, "candidate tile", i, 0, a)
                assert np.array_equal(cr[int(e["cr_offset"]) + at].reshape(-1), mine["cfl_cand"][i, 1, a + 16]), (name, "candidate tile", i, 1, a)
        for i, r in enumerate(mine["cfl_rd"]):
            lv = np.ascontiguousarray(mine["cfl_q"][i * npx:(i + 1) * npx], np.int32)
            want = int(D.rate.drv_bits(lv.ctypes.data, int(mine["cfl_eob"][i]), 1, s.ts_uv, 0, int(r["txb_skip_ctx"]), int(r["dc_sign_ctx"]), 0, 0, 0))
            assert want == int(mine["cfl_bits"][i]), (name, "rate of candidate tile", i)
        dist = mine["cfl_dist"][:, 0].reshape(-1, 2, 33) >> np.uint64(rate_util.tx_scale_shift(s.ts_uv))
        for i, job in enumerate(mine["cfl_jobs"]):
            got, masks = mg_cfl.reference_decide(D.cfl, dist[i], mine["cfl_bits"].reshape(-1, 2, 33)[i], s.alpha_bits, job)
            out["cfl"][i]["intra_chroma_mode"], out["cfl"][i]["cfl_alpha_idx"], out["cfl"][i]["cfl_alpha_signs"] = got
            out["cfl"][i]["evaluated_mask"] = masks
        if len(mine["cfl_chosen"]):
            cb, cr, _ = mg_cfl.reference_predict(D.cfl, luma, pool.cb.reshape(-1), pool.cr.reshape(-1), mine["cfl_chosen"], w, h, 8)
            out["pool_chroma"] = [cb.reshape(pool.cb.shape), cr.reshape(pool.cr.shape)]
    stage("slot_luma", "cfl", "pool_chroma")
    # 8. Av1TuCalcCostLuma, Av1FullCost / Av1MergeSkipFullCost on the slots' numbers, the loop of product_full_mode_decision
    res = mine["result"]
    slots = [k for k, sl in enumerate(st["slots"]) if sl["row"] != fu.NONE and int(res[k]["full_cost"]) != fu.U64]
    raw, post = fu.reference_leaves(D.full, _leaf_tuples(s, mine, slots, False)), fu.reference_leaves(D.full, _leaf_tuples(s, mine, slots, True))
    for i, k in enumerate(slots):
        r = res[k]
        assert (int(raw["luma"][i][0]), int(raw["luma"][i][1])) == (int(r["coeff_bits"][0]), int(r["y_distortion"][0])), (name, "Av1TuCalcCostLuma", k)
        merge = int(mine["full"][st["slots"][k]["row"]]["skip_mode_rate"]) != fu.NONE
        want = (r["full_cost"], r["merge_cost"], r["skip_cost"], r["full_lambda_rate"], 0, r["skip_flag"]) if merge else \
            (r["full_cost"], 0, 0, r["full_lambda_rate"], r["full_cost_luma"], 0)
        assert [int(v) for v in post["cost"][i]] == [int(v) for v in want], (name, "full cost", k, post["cost"][i], want)
    out["result"], out["decision"] = res, mine["decision"].copy()
    groups = [g for g in range(s.n_groups) if int(mine["decision"][g]["n_full"])]
    costs, types, modes = np.full((len(groups), 12), fu.U64, np.uint64), np.ones((len(groups), 12), np.uint8), np.zeros((len(groups), 12), np.uint8)
    for i, g in enumerate(groups):
        for j in range(int(mine["decision"][g]["n_full"])):
            r = res[g * s.max_full + j]
            costs[i, j] = r["full_cost"]
            if int(r["row"]) != fu.NONE:
                types[i, j], modes[i, j] = (1 if s.fast[int(r["row"])]["flags"] & mu.TYPE_INTER else 2), mine["full"][int(r["row"])]["intra_mode"]
    order = np.tile(np.arange(12, dtype=np.uint8), (len(groups), 1))
    ref = fu.reference_decisions(D.full, (costs, types, modes, order, mine["decision"]["n_full"][groups].astype(np.int64)))
    for i, g in enumerate(groups):
        out["decision"][g]["winner_slot"], out["decision"][g]["best_intra_mode"], out["decision"][g]["cost"] = ref[i]
    out["recon"] = mine["recon"]                                   # copies of the winners' slot tiles
    stage("result", "decision", "recon")
    return out


def main():
    from oracle.binding import Oracle
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    out = {"sizes": np.array(list(mc.SIZES), dtype="U16")}
    oracle = Oracle()
    with tempfile.TemporaryDirectory() as tmp:
        D = Drivers(tmp)
        for name in mc.SIZES:
            s, mine = mc.chain_of(name, oracle)
            m = mc.measures(s, mine)
            bad = [k for k, v in mc.conditions(name, m).items() if not v]
            assert not bad, (name, bad)
            ref = reference_chain(D, name, oracle)
            for k, v in mc.input_digests(mc.make_scenario(name)).items():
                out[f"{name}_sha256_{k}"] = v
            for k in mc.STAGES:
                if k in mc.PLANE_STAGES:
                    out[f"{name}_digest_{k}"] = mc.sha256(*ref[k])
                else:
                    out[f"{name}_{k}"] = mc.small(ref, k)
            out[f"{name}_refused"] = np.int32(mc.total_refused(mine))
            out[f"{name}_measures"] = np.array([m[k] for k in mc.MEASURES], np.int32)
            print(name, m, "refused", mc.total_refused(mine))
    save(mc.FIXTURE, out)
    print(f"wrote {mc.FIXTURE}: {os.path.getsize(mc.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
