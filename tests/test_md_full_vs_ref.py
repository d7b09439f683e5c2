"""CPU: the restatement of mode decision's full loop (tests/md_full_util.py) against tests/golden/md_full.npz -- what the reference's own
Av1TuCalcCostLuma, Av1TuCalcCost, Av1IntraFullCost, Av1InterFullCost and product_full_mode_decision returned on the constructed tuples, and
the recorded end-to-end results of the constructed cases -- and, where the reference is present, against the live driver
(tests/golden/ref_md_full_driver.c).  The cases are also checked to hold what the GPU test relies on them for."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import md_fast_util as mu  # noqa: E402
import md_full_util as fu  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


def test_leaves_equal_the_fixture():
    fx, t = fu.fixture(), fu.leaf_tuples()
    mine = fu.leaves(t)
    assert np.array_equal(mine["luma"], fx["leaf_luma"]) and np.array_equal(mine["cost"], fx["leaf_cost"])
    assert np.array_equal((t["eob"] != 0).astype(np.uint32), fx["leaf_has_coeff"])
    assert np.array_equal(fu.decisions(fu.decision_lists()), fx["decision"])
    # the tuples reach both arms of skip_cost <= merge_cost, its equality, a non-zero cost of ~0 and all-~0 cost lists
    merged = (t["inter"] != 0) & (t["merge"] != 0)
    cost = fx["leaf_cost"]
    assert (cost[merged, 5] == 1).sum() > 20 and (cost[merged, 5] == 0).sum() > 20 and (cost[merged, 1] == cost[merged, 2]).sum() > 5
    assert (cost[~merged, 1:3] == 0).all() and (cost[merged, 4] == 0).all()
    costs, _, _, order, count = fu.decision_lists()
    all_max = [i for i in range(len(costs)) if (costs[i][order[i][:count[i]]] == fu.U64).all()]
    assert len(all_max) >= 10 and all(int(fx["decision"][i][0]) == int(order[i][0]) and int(fx["decision"][i][1]) == 0xFF for i in all_max)
    ties = sum(len(set(costs[i][order[i][:count[i]]].tolist())) < count[i] for i in range(len(costs)))
    assert ties > 30


@pytest.mark.parametrize("name", list(fu.CASES))
def test_cases_equal_the_fixture(name):
    st = fu.expected(name)   # asserts the rows, the digests of the planes and the refused count
    s = fu.scenario(name)
    assert len(st["result"]) == s.n_groups * s.max_full


def test_cases_hold_what_the_gpu_test_needs():
    seen = {"invalid_picked": 0, "inactive": 0, "refused_groups": 0, "skip": 0, "merge": 0, "intra_wins": 0, "inter_wins": 0, "uv_follows": 0, "eob0": 0,
            "not_slot0": 0, "no_uv": 0, "energy": 0}
    for name in fu.CASES:
        s, st = fu.scenario(name), fu.expected(name)
        res, dec = st["result"], st["decision"]
        active = res["row"] != fu.NONE
        seen["inactive"] += int((~active).sum())
        seen["refused_groups"] += int((dec["winner_slot"] == 0xFF).sum())
        rows = res["row"][active]
        seen["invalid_picked"] += int(((s.fast["flags"][rows] & mu.INVALID) != 0).sum())
        merged = active & (res["merge_cost"] != 0)
        seen["skip"] += int((res["skip_flag"][merged] == 1).sum())
        seen["merge"] += int((res["skip_flag"][merged] == 0).sum())
        won = dec["winner_row"][dec["winner_row"] != fu.NONE]
        seen["inter_wins"] += int(((s.fast["flags"][won] & mu.TYPE_INTER) != 0).sum())
        seen["intra_wins"] += int(((s.fast["flags"][won] & mu.TYPE_INTER) == 0).sum())
        seen["not_slot0"] += int(((dec["winner_slot"] != 0) & (dec["winner_slot"] != 0xFF)).sum())
        if (s.mask_inter | s.mask_intra) != 1:
            inter = active & ((s.fast["flags"][np.where(active, res["row"], 0)] & mu.TYPE_INTER) != 0)
            assert (res["tx_type_uv"][inter] == res["tx_type_y"][inter]).all()
            seen["uv_follows"] += int((res["tx_type_y"][inter] != 0).sum())
        seen["eob0"] += int((active & (res["eob"][:, 0] == 0) & (res["full_cost"] != fu.U64)).sum())
        seen["no_uv"] += int((s.fast["has_uv"][rows] == 0).sum())
        seen["energy"] += sum(st["luma"][k]["energy"] > 0 for k in range(s.n_slots))
        assert int((dec["winner_slot"] == 0xFF).sum()) == st["refused"]
    assert all(v > 0 for v in seen.values()), seen
    s4 = fu.scenario("4x4")
    assert {0, 1} <= set(s4.fast["has_uv"].tolist())
    assert fu.scenario("8x8_g23_m12").n_slots == 276 and fu.scenario("16x8_g5_m1").max_full == 1


@pytest.mark.skipif(not reference_available(), reason="the reference is not on this machine")
def test_restatement_equals_the_live_reference(tmp_path):
    L = fu.build_reference_driver(str(tmp_path))
    t, lists = fu.leaf_tuples(150, seed=77), fu.decision_lists(60, seed=78)
    ref, mine = fu.reference_leaves(L, t), fu.leaves(t)
    assert np.array_equal(ref["luma"], mine["luma"]) and np.array_equal(ref["cost"], mine["cost"])
    assert np.array_equal(ref["has_coeff"], (t["eob"] != 0).astype(np.uint32))
    assert np.array_equal(fu.reference_decisions(L, lists), fu.decisions(lists))
