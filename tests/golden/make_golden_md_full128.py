"""Writes tests/golden/md_full128.npz from the reference's own ProductFullLoop, FullLoop_R, CuFullDistortionFastTuMode_R, Av1InterFullCost /
Av1IntraFullCost and AV1PerformInverseTransformRecon on blocks of 128x128, 128x64 and 64x128 (tests/golden/ref_md_full128_driver.c, linked
by the recipe of oracle/ref_driver.py against the reference objects of the oracle build, oracle/_ref/obj_all).  Run in the build container
only, where the reference exists: the fixture is data.

    python tests/golden/make_golden_md_full128.py

All five functions run stand-alone, whole, each with its own loop over txb_itr, on the reference's own BlockGeom (build_blk_geom), so
nothing of them is restated for the fixture.  What the driver does not run is AV1PerformFullLoop around them (it needs the encoder's
constructors): the order ProductFullLoop -> FullLoop_R -> CuFullDistortionFastTuMode_R -> full cost is the driver's, block_has_coeff
(Codec/EbProductCodingLoop.c:2229) is not compared, and the loop of product_full_mode_decision is the one tests/golden/md_full.npz pins.

The inputs are constructed (tests/md_full128_util.py: scenario) and are not stored.  Contents, per case of md_full128_util.CASES:
  {case}__geometry [1 + 8 + 2] i32   the reference's txb_count, tx_org_x / tx_org_y of four TUs, txsize[0], txsize_uv[0]
  {case}__ref_slots [n] i32          the slots with a cost: the candidates the reference ran on
  {case}__ref64 [n][15] u64          y / cb / cr distortion [2] each, coefficient bits [3], full cost, merge cost, skip cost, full_lambda_rate,
                                     full_cost_luma, the last TU's three_quad_energy
  {case}__ref32 [n][19] i32          eob[3][4], quantized_dc[3], y_ / u_ / v_has_coeff, skip_flag
  {case}__ref_recon [n]              SHA-256 of the block AV1PerformInverseTransformRecon leaves (Y, Cb, Cr)
  {case}__result, __tu, __decision   the restatement's svthip_md_full_result / svthip_md_full128_tu / svthip_md_full_decision rows, as bytes
  {case}__per_tu [slots][TUs][16]    the restatement's numbers per TU (md_full128_util.per_tu_numbers)
  {case}__digests, __refused         SHA-256 of the slot planes and of the reconstructed picture after the call, the refused count
While it writes, the restatement is asserted equal to the reference on every slot with a cost, and the coverage conditions below are
asserted of those results."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "svt-av1-1_amd", "python")]

import md_full128_util as wu  # noqa: E402
import md_full_util as fu  # noqa: E402
from make_golden_cdef import save  # noqa: E402
from oracle.binding import Oracle  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

PER_SIZE = ("y mask partial",)   # asserted of every case; the other conditions of some case


def reference_entries(L, s, st):
    """the reference on every slot of a restated call that has a cost; asserts the restatement equal to it -> the fixture's arrays"""
    n_tu, org, ts_y, ts_uv = wu.reference_geometry(L, s.w, s.h)
    assert org == s.origins and (ts_y, ts_uv) == (wu.TS_Y, wu.TS_UV), "the reference's geometry is not the restatement's"
    slots = [k for k in range(s.n_slots) if int(st["result"][k]["full_cost"]) != wu.U64]
    ref64, ref32, digests = np.zeros((len(slots), 15), np.uint64), np.zeros((len(slots), 19), np.int32), []
    for i, k in enumerate(slots):
        ref64[i], ref32[i], recon = wu.reference_slot(L, s, st["slots"][k]["row"])
        mine64, mine32, tiles = wu.restated_slot(s, st, k)
        assert np.array_equal(ref64[i], mine64) and np.array_equal(ref32[i], mine32), (s.name, k, ref64[i], mine64, ref32[i], mine32)
        assert all(np.array_equal(a, b) for a, b in zip(recon, tiles)), (s.name, k, "the reconstruction differs from the reference's")
        digests.append(fu.digest(recon))
    geometry = np.array([n_tu] + [v for o in (org + [(0, 0)] * 4)[:4] for v in o] + [ts_y, ts_uv], np.int32)
    return {"geometry": geometry, "ref_slots": np.array(slots, np.int32), "ref64": ref64, "ref32": ref32, "ref_recon": np.array(digests)}


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    out, covered = {}, {}
    oracle = Oracle()
    with tempfile.TemporaryDirectory() as tmp:
        L = wu.build_reference_driver(tmp)
        for name in wu.CASES:
            s = wu.scenario(name)
            st = wu.full_loop(oracle, s)
            for key, v in reference_entries(L, s, st).items():
                out[f"{name}__{key}"] = v
            cov = wu.coverage(s, st)
            for key in PER_SIZE:
                assert cov[key], f"{name}: no slot with: {key}"
            for key, v in cov.items():
                covered[key] = covered.get(key, False) or v
            out[f"{name}__result"] = np.frombuffer(st["result"].tobytes(), np.uint8)
            out[f"{name}__tu"] = np.frombuffer(st["tu"].tobytes(), np.uint8)
            out[f"{name}__decision"] = np.frombuffer(st["decision"].tobytes(), np.uint8)
            out[f"{name}__per_tu"] = wu.per_tu_numbers(s, st)
            out[f"{name}__digests"] = np.array([fu.digest(st["slot"]), fu.digest(st["recon"])])
            out[f"{name}__refused"] = np.array(st["refused"], np.int32)
    missing = [k for k, v in covered.items() if not v]
    assert not missing, f"the constructed inputs do not cover: {missing}"
    path = os.path.join(HERE, "md_full128.npz")
    save(path, out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
