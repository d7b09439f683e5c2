"""CPU: the restatement of the restoration decision (tests/lr_finish_util.py) against tests/golden/lr_finish.npz, which holds what the
reference's own rest_finish_search (Codec/EbRestorationPick.c:1971-2040) made of the constructed cases and of the three chain pictures'
search tables; where the reference is available, against the driver itself, with the bit-count leaves on an exhaustive (ref, v) grid per
coded symbol; and the issue's coverage list on the committed fixture."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), ROOT]

import lr_finish_util as fu  # noqa: E402
import post_filter_chain_util as pc  # noqa: E402

CHAIN = ("A", "B", "C")


def test_restatement_matches_fixture_on_every_case():
    """unit types, best_rtype of the three walks, sse, bits, frame_type, n_tried, and cost by bit pattern"""
    assert fu.n_cases() >= 54
    for i in range(fu.n_cases()):
        F = fu.fixture_case(i)
        mine = fu.finish(F["rates"], F["unit_base"], *[F[k] for k in fu.INPUT_KEYS])
        diff = fu.first_difference(mine, F)
        assert diff is None, f"case {i} ({F['name']}): {diff}"


def test_fixture_is_what_the_cases_are_built_from():
    """the committed tables are the constructed cases of lr_finish_util, so the coverage below speaks of what the generator fed the reference"""
    cases = fu.constructed_cases()
    assert [c["name"] for c in cases] == [str(n) for n in fu.fixture()["names"]]
    for i, c in enumerate(cases):
        F = fu.fixture_case(i)
        assert F["geom"] == c["geom"] and F["rates"] == c["rates"] and F["range"] == tuple(c["range"]), c["name"]
        assert F["unit_base"] == fu.unit_base_of(fu.unit_counts(*c["geom"])), c["name"]
        assert all(np.array_equal(F[k], c[k]) for k in fu.INPUT_KEYS), c["name"]


@pytest.mark.parametrize("name", CHAIN)
def test_restatement_matches_fixture_on_the_chain_pictures(name):
    want = pc.expected(name)
    _, base = pc.lu.picture_units(pc.W, pc.H)
    assert 1 <= len(fu.chain_settings(name)) <= 4
    for k, s in enumerate(fu.chain_settings(name)):
        assert s[0] in fu.CHAIN_RDMULT and s[1] in fu.CHAIN_X
        F = fu.chain_case(name, k)
        mine = fu.finish(F["rates"], base, *[want[key] for key in fu.INPUT_KEYS])
        diff = fu.first_difference(mine, F)
        assert diff is None, f"picture {name}, setting {s}: {diff}"


def test_fixture_covers_the_issues_list():
    """re-asserted on the committed fixture, from the reference's outputs stored there"""
    cov = fu.coverage([fu.fixture_case(i) for i in range(fu.n_cases())])
    assert len(cov) == 17
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    # the chain pictures
    z = fu.fixture()
    _, base = pc.lu.picture_units(pc.W, pc.H)
    at = {n: {s: k for k, s in enumerate(fu.chain_settings(n))} for n in CHAIN}
    assert {int(t) for n in CHAIN for t in z[f"{n}_frame_type"].reshape(-1)} == {0, 1, 2, 3}
    for n, s in (("B", (10_000_000, 1 << 22)), ("C", (2_000_000, 1 << 18))):
        ut = z[f"{n}_unit_type"][at[n][s]]
        assert any(set(ut[base[p]:base[p + 1]].tolist()) == {0, 1, 2} for p in (1, 2)), (n, s)
    assert 0 in z["A_frame_type"][at["A"][(10_000_000, 1 << 22)]].tolist()
    assert 2 in z["A_frame_type"][at["A"][(60000, 1 << 26)]].tolist()


def test_leaf_counts_match_fixture():
    z = fu.fixture()
    for j in range(len(z["leaf_win"])):
        assert fu.count_wiener_bits(int(z["leaf_win"][j]), z["leaf_taps"][j].tolist(), z["leaf_ref"][j].tolist()) == int(z["leaf_wiener_bits"][j])
        assert fu.count_sgrproj_bits(int(z["leaf_sgr"][j][0]), z["leaf_sgr"][j][1:].tolist(), z["leaf_sgr_ref"][j].tolist()) == int(z["leaf_sgr_bits"][j])


def test_rounding_case_is_one():
    """the two candidates of the rounding case differ in exact arithmetic and are the same double (Python integers against floats)"""
    F = next(fu.fixture_case(i) for i in range(fu.n_cases()) if fu.fixture_case(i)["name"] == "rounding")
    r, dflt = F["rates"], list(fu.TAP_MID) * 2
    assert r["rdmult"] % 2 == 1 and int(F["wiener_sse"][0, 0]) >= 1 << 38
    bits = r["wiener_cost"][1] + (fu.count_wiener_bits(7, fu.coded_taps(F["taps"][0]), dflt) << fu.COST_SHIFT)
    none, wi = int(F["wiener_sse"][0, 0]), int(F["wiener_sse"][0, 1])
    assert fu.rdcost_exact(r["rdmult"], bits, wi) < fu.rdcost_exact(r["rdmult"], r["wiener_cost"][0], none)
    assert fu.rdcost(r["rdmult"], bits, wi) == fu.rdcost(r["rdmult"], r["wiener_cost"][0], none)
    assert F["best_rtype"][0, 0] == fu.NONE          # integer arithmetic would have taken Wiener


def _reference_available():
    from oracle.ref_driver import reference_available
    return reference_available()


@pytest.mark.skipif(not _reference_available(), reason="needs the reference's sources and the oracle build (the build container); the fixture stands in")
def test_against_the_driver_directly(tmp_path):
    """every constructed case live through rest_finish_search, and the bit counts for every (ref, v) of every coded symbol"""
    import make_golden_lr_finish as mg
    L = mg.build_driver(str(tmp_path))
    for c in fu.constructed_cases():
        counts = mg.open_geometry(L, *c["geom"])
        base = fu.unit_base_of(counts)
        tables = tuple(c[k] for k in fu.INPUT_KEYS)
        ref = mg.reference_finish(L, c["rates"], base, *tables)
        L.drv_lr_close()
        assert counts == fu.unit_counts(*c["geom"])
        diff = fu.first_difference(fu.finish(c["rates"], base, *tables), ref)
        assert diff is None, f"{c['name']}: {diff}"
    dflt, prj = list(fu.TAP_MID) * 2, list(fu.PRJ_MID)
    for j in range(6):                       # one tap at a time over its whole (ref, v) grid, the others at their defaults
        lo, hi = fu.TAP_MIN[j % 3], fu.TAP_MAX[j % 3]
        grid = [(r, v) for r in range(lo, hi + 1) for v in range(lo, hi + 1)]
        taps, refs = np.tile(dflt, (len(grid), 1)), np.tile(dflt, (len(grid), 1))
        refs[:, j], taps[:, j] = [g[0] for g in grid], [g[1] for g in grid]
        for win in (7, 5):
            wb, _ = mg.reference_bits(L, np.full(len(grid), win), taps, refs, np.tile([0] + prj, (len(grid), 1)), np.tile(prj, (len(grid), 1)))
            assert wb.tolist() == [fu.count_wiener_bits(win, t.tolist(), r.tolist()) for t, r in zip(taps, refs)], (j, win)
    for k in range(2):
        lo, hi = fu.PRJ_MIN[k], fu.PRJ_MAX[k]
        grid = [(r, v) for r in range(lo, hi + 1) for v in range(lo, hi + 1)]
        for ep in (0, 12, 15):
            sgr, refs = np.tile([ep] + prj, (len(grid), 1)), np.tile(prj, (len(grid), 1))
            refs[:, k], sgr[:, 1 + k] = [g[0] for g in grid], [g[1] for g in grid]
            _, sb = mg.reference_bits(L, np.full(len(grid), 7), np.tile(dflt, (len(grid), 1)), np.tile(dflt, (len(grid), 1)), sgr, refs)
            assert sb.tolist() == [fu.count_sgrproj_bits(ep, s[1:].tolist(), r.tolist()) for s, r in zip(sgr, refs)], (k, ep)
