"""Writes tests/golden/post_filter_chain128.npz from the reference's own stages run as a chain on pictures coded with 128-wide blocks:
av1_pick_filter_level -> av1_loop_filter_frame -> cdef_seg_search / finish_cdef_search -> av1_cdef_frame, each fed what the reference's
stage before it left.  The drivers and the calls are those of make_golden_dlf.py and make_golden_cdef128.py; this file holds no reference
text.  Run in the build container only, where the reference exists: the fixture is data.

    python tests/golden/make_golden_post_filter_chain128.py

At every stage the restated chain (tests/post_filter_chain128_util.py) is asserted equal to the reference's.
Contents, per picture n of post_filter_chain128_util.PICTURES (328 x 200; regenerated from their seeds, not stored)
  {n}_seed, {n}_bd, {n}_last_levels, {n}_base_qindex     the parameters
  {n}_sha256_recon, {n}_sha256_source, {n}_sha256_mi     sha256 of the generated inputs
  {n}_levels, {n}_masks                    the four picked levels; the levels each of the five walks tried, as bit masks
  {n}_mse, {n}_counted                     [2][nfb][64] cdef_seg_search's tables; [nfb] 1 for a searched fb
  {n}_cdef_result, {n}_fb_strength         finish_cdef_search's result as 21 int32; [nfb] cdef_strength of each fb's first cell, -1 untouched
  {n}_digest_dbk, {n}_digest_cdef          film_grain_util.digest of the three planes after each stage
  {n}_dbk_d{p}, {n}_cdef_d{p}              the planes whole, each minus the stage before it (dbk minus the reconstruction)"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import cdef_util as cu  # noqa: E402
import make_golden_cdef as mg_cdef  # noqa: E402
import make_golden_cdef128 as mg_cdef128  # noqa: E402
import make_golden_dlf as mg_dlf  # noqa: E402
import make_golden_lr as mg_lr  # noqa: E402
import post_filter_chain128_util as pc128  # noqa: E402
import post_filter_chain_util as pc  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


class Drivers:
    def __init__(self, tmp):
        def sub(name):
            d = os.path.join(tmp, name)
            os.makedirs(d)
            return d
        self.dlf, self.cdef = mg_dlf.build_driver(sub("dlf")), mg_cdef128.build_driver(sub("cdef128"))


def reference_chain(D, recon, source, mi, bd, last_levels, base_qindex, mine=None):
    """the reference's own stages as a chain, by the names of post_filter_chain128_util.run_chain; `mine` is compared stage by stage"""
    out = {}

    def stage(*keys):
        if mine is not None:
            diff = pc128.first_difference(mine, out, only=keys)
            assert diff is None, "the restated chain differs from the reference's chain at " + diff

    levels, trace = mg_dlf.reference_pick(D.dlf, bd, mi, recon, source, last_levels, 0)
    _, masks, my_trace = pc128.du.pick_filter_level(recon, source, mi, last_levels, 0, 0, bd)
    assert np.array_equal(np.array(my_trace), trace), "the restatement's pick ran other filterings than the reference's"
    out["levels"], out["masks"] = np.array(levels, np.int32), np.array(masks, np.uint64)
    out["dbk"] = mg_dlf.reference_filter(D.dlf, bd, mi, recon, levels, 0, 0, 3)
    stage("levels", "masks", "dbk")
    skip, sb = pc128.grids(mi)
    R = mg_cdef128.Reference(D.cdef, pc128.W, pc128.H, bd, out["dbk"], source, skip, sb)
    out["mse"] = R.search(base_qindex)
    res, fbs = R.finish(base_qindex)
    out["counted"] = pc128.c128.layout(sb, skip, pc128.W, pc128.H)[0].reshape(-1).astype(np.uint8)     # which rows the search filled
    assert not out["mse"][:, out["counted"] == 0].any() and int(res["sb_count"]) == int(out["counted"].sum())
    out["cdef_result"], out["fb_strength"] = res.reshape(1).view(np.int32).copy(), fbs
    out["cdef"] = R.frame(res, fbs)
    R.close()
    stage("mse", "counted", "cdef_result", "fb_strength", "cdef")
    return out


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    out = {"pictures": np.array(list(pc128.PICTURES), dtype="U1")}
    with tempfile.TemporaryDirectory() as tmp:
        D = Drivers(tmp)
        for name, P in pc128.PICTURES.items():
            mi, recon, source, mine = pc128.chain_of(name)
            bad = [k for k, v in pc128.conditions(recon, mine).items() if not v]
            assert not bad, (name, bad)
            ref = reference_chain(D, recon, source, mi, P["bd"], P["last_levels"], P["base_qindex"], mine=mine)
            for k in pc128.PARAM_KEYS:
                out[f"{name}_{k}"] = np.int32(P[k])
            out[f"{name}_last_levels"] = np.array(P["last_levels"], np.int32)
            for k, v in pc.input_digests(mi, recon, source).items():
                out[f"{name}_sha256_{k}"] = v
            for k, dt in pc128.SMALL:
                out[f"{name}_{k}"] = np.ascontiguousarray(ref[k]).astype(dt)
            prev = recon
            for k in pc128.PLANE_STAGES:
                out[f"{name}_digest_{k}"] = pc.plane_digest(ref[k])
                for p in range(3):
                    out[f"{name}_{k}_d{p}"] = mg_lr.delta(ref[k][p], prev[p])
                prev = ref[k]
            res = ref["cdef_result"].view(cu.RESULT_DTYPE)[0]
            print("picture", name, "levels", ref["levels"].tolist(), "cdef_bits", int(res["cdef_bits"]), "counted", ref["counted"].tolist(),
                  "fb_strength", ref["fb_strength"].tolist(), flush=True)
    mg_cdef.save(pc128.FIXTURE, out)
    print(f"wrote {pc128.FIXTURE}: {os.path.getsize(pc128.FIXTURE)} bytes")
    assert os.path.getsize(pc128.FIXTURE) < 970_000


if __name__ == "__main__":
    main()
