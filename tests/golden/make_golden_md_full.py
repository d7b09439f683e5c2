"""Writes tests/golden/md_full.npz from the reference's own Av1TuCalcCostLuma, Av1TuCalcCost, Av1IntraFullCost, Av1InterFullCost and
product_full_mode_decision (tests/golden/ref_md_full_driver.c, linked by the recipe of oracle/ref_driver.py against the reference objects of
the oracle build, oracle/_ref/obj_all).  Run in the build container only, where the reference exists: the fixture is data.

    python tests/golden/make_golden_md_full.py

The inputs are constructed (tests/md_full_util.py: leaf_tuples, decision_lists, scenario) and are not stored.  Contents:
  leaf_luma [300][3] u64       Av1TuCalcCostLuma on leaf_tuples(): yTuCoeffBits, yTuDistortion[DIST_CALC_RESIDUAL], yFullCost
  leaf_cost [300][6] u64       Av1IntraFullCost / Av1InterFullCost: full cost, merge cost, skip cost, full_lambda_rate, full_cost_luma, skip_flag
  leaf_has_coeff [300][3] u32  y_has_coeff of Av1TuCalcCostLuma, u_ / v_has_coeff of Av1TuCalcCost(COMPONENT_CHROMA)
  decision [120][3] u64        product_full_mode_decision on decision_lists(): lowestCostIndex, best_intra_mode, the block's cost
  {case}__result, __decision   the restatement's svthip_md_full_result / _decision rows of md_full_util.CASES, as bytes
  {case}__digests, __refused   SHA-256 of the slot planes and of the reconstructed picture after the call, the refused count
While it writes, the restatement is asserted equal to the reference on every leaf.  What the reference cannot be run for without the
encoder's constructors -- AV1PerformFullLoop around these leaves -- is the restatement's, on top of the chain and the rate that
tests/test_tq_vs_ref.py and tests/test_coeff_rate_vs_ref.py pin."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "svt-av1-1_amd", "python")]

import md_full_util as fu  # noqa: E402
from make_golden_cdef import save  # noqa: E402
from oracle.binding import Oracle  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = fu.build_reference_driver(tmp)
        t, lists = fu.leaf_tuples(), fu.decision_lists()
        ref, mine = fu.reference_leaves(L, t), fu.leaves(t)
        assert np.array_equal(ref["luma"], mine["luma"]) and np.array_equal(ref["cost"], mine["cost"]), "the restatement differs from the reference"
        assert np.array_equal(ref["has_coeff"], (t["eob"] != 0).astype(np.uint32))
        dec = fu.reference_decisions(L, lists)
        assert np.array_equal(dec, fu.decisions(lists)), "the restated decision loop differs from the reference"
        merged = (t["inter"] != 0) & (t["merge"] != 0)
        assert (ref["cost"][merged, 5] == 1).sum() > 20 and (ref["cost"][merged, 5] == 0).sum() > 20 and (ref["cost"][merged, 1] == ref["cost"][merged, 2]).sum() > 5
        out.update(leaf_luma=ref["luma"], leaf_cost=ref["cost"], leaf_has_coeff=ref["has_coeff"], decision=dec)
    oracle = Oracle()
    for name in fu.CASES:
        st = fu.full_loop(oracle, fu.scenario(name))
        out[f"{name}__result"] = np.frombuffer(st["result"].tobytes(), np.uint8)
        out[f"{name}__decision"] = np.frombuffer(st["decision"].tobytes(), np.uint8)
        out[f"{name}__digests"] = np.array([fu.digest(st["slot"]), fu.digest(st["recon"])])
        out[f"{name}__refused"] = np.array(st["refused"], np.int32)
    path = os.path.join(HERE, "md_full.npz")
    save(path, out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
