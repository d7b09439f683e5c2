"""Writes tests/golden/post_filter_chain.npz from the reference's own post-reconstruction stages run as a chain: av1_pick_filter_level ->
av1_loop_filter_frame -> cdef_seg_search / finish_cdef_search -> av1_cdef_frame -> search_wiener_seg, search_sgrproj_seg ->
av1_loop_restoration_filter_frame -> av1_add_film_grain_run, each fed what the reference's stage before it left.  The drivers and the
calls are those of make_golden_dlf.py, make_golden_cdef.py, make_golden_lr.py, make_golden_lr_sgr.py and make_golden_film_grain.py; this
file holds no reference text.  Run in the build container only, where the reference exists: the fixture is data.

    python tests/golden/make_golden_post_filter_chain.py

At every stage the restated chain (tests/post_filter_chain_util.py) is asserted equal to the reference's, so a restatement that errs at
inputs its own fixture never had stops the generator.  The restoration unit types are post_filter_chain_util.unit_types (u % 3), the
taps and self-guided parameters the reference searches' own.

Contents, per picture n of post_filter_chain_util.PICTURES (200 x 200; regenerated from their seeds, not stored)
  {n}_seed, {n}_bd, {n}_last_levels, {n}_base_qindex, {n}_grain_set   the parameters
  {n}_sha256_recon, {n}_sha256_source, {n}_sha256_mi                  sha256 of the generated inputs
  {n}_levels, {n}_masks                    the four picked levels; the levels each of the five walks tried, as bit masks
  {n}_mse, {n}_counted                     [2][nfb][64] cdef_seg_search's tables; [nfb] sb_all_skip is false
  {n}_cdef_result, {n}_fb_strength         finish_cdef_search's result as 21 int32 (cdef_util.RESULT_DTYPE); [nfb] picked index, -1 left out
  {n}_wiener_sse, {n}_taps, {n}_n_trials   [units][2] sse[RESTORE_NONE], sse[RESTORE_WIENER]; [units][16] the taps search_wiener_seg left;
                                           the number of trial filters
  {n}_sgrproj, {n}_sgr_sse                 [units][4] ep, xqd0, xqd1, 0; [units] sse[RESTORE_SGRPROJ]
  {n}_unit_type                            [units] the types the frame filter ran with
  {n}_digest_dbk, _cdef, _restored, _grain film_grain_util.digest of the three planes after each stage
  A_dbk_d{p}, A_cdef_d{p}, A_restored_d{p}, A_grain_d{p}   picture A's planes whole, each minus the stage before it (dbk minus the
                                           reconstruction); post_filter_chain_util.expected adds them up
The reference's leaf functions are its dispatched SIMD forms, as in the five fixtures of the single stages."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import cdef_util as cu  # noqa: E402
import film_grain_util as fu  # noqa: E402
import lr_util as lu  # noqa: E402
import make_golden_cdef as mg_cdef  # noqa: E402
import make_golden_dlf as mg_dlf  # noqa: E402
import make_golden_film_grain as mg_fg  # noqa: E402
import make_golden_lr as mg_lr  # noqa: E402
import make_golden_lr_sgr as mg_sgr  # noqa: E402
import post_filter_chain_util as pc  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

WHOLE = ("A",)      # the pictures whose planes are kept whole
SIZE_LIMIT = 970_000


class Drivers:
    """the four reference drivers, each built in a directory of its own under `tmp`"""

    def __init__(self, tmp):
        def sub(name):
            d = os.path.join(tmp, name)
            os.makedirs(d)
            return d
        self.dlf, self.cdef, self.fg = mg_dlf.build_driver(sub("dlf")), mg_cdef.build_driver(sub("cdef")), mg_fg.build_driver(sub("fg"))
        self.lr = mg_sgr.build_driver(sub("lr"))                 # ref_lr_sgr_driver.c includes ref_lr_driver.c: both searches, one filter
        self.lr.drv_lr_search.argtypes = [C.c_int] + [C.c_void_p] * 10


def reference_chain(D, recon, source, mi, bd, last_levels, base_qindex, grain_set, w=pc.W, h=pc.H, mine=None):
    """the reference's own stages as a chain, by the names of post_filter_chain_util.run_chain.  `mine` (the restated chain): compared
    stage by stage as soon as the reference's stage is there, so the first restatement that differs is the one named"""
    out = {}

    def stage(*keys):
        if mine is not None:
            diff = pc.first_difference(mine, out, only=keys)
            assert diff is None, "the restated chain differs from the reference's chain at " + diff

    levels, trace = mg_dlf.reference_pick(D.dlf, bd, mi, recon, source, last_levels, 0)
    _, masks, my_trace = pc.du.pick_filter_level(recon, source, mi, last_levels, 0, 0, bd)
    assert np.array_equal(np.array(my_trace), trace), "the restatement's pick ran other filterings than the reference's"
    out["levels"], out["masks"] = np.array(levels, np.int32), np.array(masks, np.uint64)     # the masks: split from the (equal) trace
    out["dbk"] = mg_dlf.reference_filter(D.dlf, bd, mi, recon, levels, 0, 0, 3)
    stage("levels", "masks", "dbk")

    skip = pc.skip_map(mi, w, h)
    R = mg_cdef.Reference(D.cdef, w, h, bd, out["dbk"], source, skip)
    out["mse"] = R.search(base_qindex)
    res, fbs = R.finish(base_qindex)
    out["counted"], out["cdef_result"], out["fb_strength"] = (fbs >= 0).astype(np.uint8), res.reshape(1).view(np.int32).copy(), fbs
    out["cdef"] = R.frame(res, fbs)
    R.close()
    stage("mse", "counted", "cdef_result", "fb_strength", "cdef")

    R = mg_lr.Reference(D.lr, w, h, bd, out["cdef"], out["dbk"], source)
    limits, _ = R.units()
    planes, base = lu.picture_units(w, h)
    assert all(np.array_equal(limits[p], planes[p][0]) for p in range(3)), "geometry differs from the reference's"
    n_units = [len(v) for v in limits]
    wiener, sgr = R.search(n_units), mg_sgr.reference_search(R, n_units, False)
    out["wiener_sse"], out["taps"] = np.concatenate([r["sse"] for r in wiener]), np.concatenate([r["final"] for r in wiener])
    out["n_trials"] = np.concatenate([r["n_trials"] for r in wiener])
    out["rejected"] = np.concatenate([r["rejected"] for r in wiener]) != 0
    out["sgrproj"], out["sgr_sse"] = np.concatenate([r["sgrproj"] for r in sgr]), np.concatenate([r["sse"] for r in sgr])
    out["unit_type"] = pc.unit_types(base[3])
    out["restored"] = mg_sgr.reference_filter(R, (1, 1, 1), base, out["unit_type"], out["taps"], out["sgrproj"])
    R.close()
    stage("wiener_sse", "taps", "n_trials", "sgrproj", "sgr_sse", "unit_type", "restored")

    out["grain"] = mg_fg.reference_run(D.fg, fu.PARAM_SETS[grain_set], bd, out["restored"])
    stage("grain")
    return out


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    out = {"pictures": np.array(list(pc.PICTURES), dtype="U1"), "whole": np.array(WHOLE, dtype="U1")}
    with tempfile.TemporaryDirectory() as tmp:
        D = Drivers(tmp)
        for name, P in pc.PICTURES.items():
            mi, recon, source, mine = pc.chain_of(name)
            bad = [k for k, v in pc.conditions(name, recon, mine).items() if not v]
            assert not bad, (name, bad)
            assert not mine["rejected"].any(), (name, "a Wiener unit is rejected: its type would filter with no taps")
            ref = reference_chain(D, recon, source, mi, P["bd"], P["last_levels"], P["base_qindex"], P["grain_set"], mine=mine)
            for k in pc.PARAM_KEYS:
                out[f"{name}_{k}"] = np.int32(P[k])
            out[f"{name}_last_levels"] = np.array(P["last_levels"], np.int32)
            for k, v in pc.input_digests(mi, recon, source).items():
                out[f"{name}_sha256_{k}"] = v
            for k, dt in pc.SMALL:
                out[f"{name}_{k}"] = np.ascontiguousarray(ref[k]).astype(dt)
            prev = recon
            for k in pc.PLANE_STAGES:
                out[f"{name}_digest_{k}"] = pc.plane_digest(ref[k])
                if name in WHOLE:
                    for p in range(3):
                        out[f"{name}_{k}_d{p}"] = mg_lr.delta(ref[k][p], prev[p])
                prev = ref[k]
            res = ref["cdef_result"].view(cu.RESULT_DTYPE)[0]
            print("picture", name, "levels", ref["levels"].tolist(), "cdef_bits", int(res["cdef_bits"]), "left out", int((ref["fb_strength"] == -1).sum()),
                  "Wiener trials", ref["n_trials"].tolist(), "sets", ref["sgrproj"][:, 0].tolist(),
                  "changed", {k: [int((a != b).sum()) for a, b in zip(x, y)] for k, x, y in
                              zip(pc.PLANE_STAGES, [ref[k] for k in pc.PLANE_STAGES], [recon] + [ref[k] for k in pc.PLANE_STAGES])})
    mg_cdef.save(pc.FIXTURE, out)
    mg_lr.print_sizes(out)
    print(f"wrote {pc.FIXTURE}: {os.path.getsize(pc.FIXTURE)} bytes")
    assert os.path.getsize(pc.FIXTURE) < SIZE_LIMIT


if __name__ == "__main__":
    main()
