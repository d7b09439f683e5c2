"""The numpy restatement of the in-loop motion estimation (tests/me_inloop_util.py) against tests/golden/inloop_me.npz, which holds what the
reference's own in_loop_motion_estimation_sblock leaves (use_subpel_flag = 0), and against the live driver where the reference is built;
and the generated index tables (no GPU needed)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), ROOT]

import me_inloop_util as iu  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


TRACES = []   # (quarter-pel method, psub_pel_direction) of every refined block, filled by test_restatement_equals_the_reference


@pytest.fixture(scope="module")
def cases():
    return iu.fixture_cases(iu.load_fixture())


def test_fixture_holds_the_cases_the_generator_makes(cases):
    made = iu.make_cases()
    assert [c[0] for c in cases] == [c[0] for c in made] == ["random", "small_odd", "largest", "flat", "extreme", "shifted"]
    for (_, src, refs, ctr, aw, ah, _), (_, m_src, m_refs, m_ctr, m_aw, m_ah) in zip(cases, made):
        assert np.array_equal(src, m_src) and all(np.array_equal(a, b) for a, b in zip(refs, m_refs)) and np.array_equal(ctr, m_ctr) and (aw, ah) == (m_aw, m_ah)


@pytest.mark.parametrize("index", range(6))
def test_restatement_equals_the_reference(cases, index):
    name, src, refs, ctr, aw, ah, want = cases[index]
    got = iu.restate_case(src, refs, ctr, aw, ah)
    for k in ("desc", "best_sad", "best_mv", "inloop_mv"):
        assert np.array_equal(got[k], want[k]), (name, k)
    trace = []
    sub = iu.restate_case(src, refs, ctr, aw, ah, use_subpel=True, trace=trace)
    keep = ~want["sub_stale"]
    for k in ("best_sad", "best_mv"):
        assert np.array_equal(sub[k][keep], want["sub_" + k][keep]), (name, "sub-pel", k)
    assert np.array_equal(sub["inloop_mv"][keep[:, :, iu.PACK_SOURCE]], want["sub_inloop_mv"][keep[:, :, iu.PACK_SOURCE]]), (name, "sub-pel inloop_mv")
    TRACES.extend(trace)
    # the 136 blocks of the four shapes neither walk visits keep their full-pel result
    unrefined = np.array([(int(w), int(h)) in iu.NOT_REFINED for _, _, w, h in iu.BLOCKS])
    assert int(unrefined.sum()) == 136 and np.array_equal(want["sub_best_mv"][:, :, unrefined], want["best_mv"][:, :, unrefined]), name


def test_every_quarter_pel_method_and_direction_is_taken(cases):
    trace = list(TRACES)
    if not trace:   # run alone: restate the shifted case
        name, src, refs, ctr, aw, ah, _ = cases[5]
        iu.restate_case(src, refs, ctr, aw, ah, use_subpel=True, trace=trace)
    assert {m for m, _ in trace} == {0, 1, 2, 3} and {d for _, d in trace} == set(range(8))


def test_fixture_properties(cases):
    by_name = {c[0]: c for c in cases}
    sizes = {(int(d[4]), int(d[5])) for d in by_name["random"][6]["desc"].reshape(-1, 8)}
    assert any(w == 1 for w, _ in sizes) and any(h == 1 for _, h in sizes) and any(w % 4 for w, _ in sizes if w > 1)
    flat = by_name["flat"][6]
    assert (flat["best_mv"] == flat["best_mv"][:, :, :1]).all()                 # every SAD ties: the first raster position wins for every block
    assert int(by_name["extreme"][6]["best_sad"][0, 0, 340]) == 64 * 64 * 255    # the 20-bit SAD
    assert not any(c[6]["sub_stale"].any() for c in cases)   # no block of the fixture depends on bytes the reference never wrote
    assert {(int(d[4]), int(d[5])) for d in by_name["largest"][6]["desc"].reshape(-1, 8)} == {(127, 127)}


@pytest.mark.skipif(not reference_available(), reason="needs the reference sources and oracle/_ref/obj_all")
def test_live_reference_equals_the_fixture(cases, tmp_path):
    import make_golden_inloop_me as gen
    L = gen.build_driver(str(tmp_path))
    for name, src, refs, ctr, aw, ah, want in cases:
        ref = gen.reference_case(L, src, refs, ctr, aw, ah)
        assert np.array_equal(ref["origin"], want["desc"][:, :, 2:4]), name
        for k in ("best_sad", "best_mv", "inloop_mv"):
            assert np.array_equal(ref[k], want[k]), (name, k)
        sub = gen.reference_case(L, src, refs, ctr, aw, ah, use_subpel=1)
        assert np.array_equal(sub["stale"], want["sub_stale"]), name
        for k in ("best_sad", "best_mv", "inloop_mv"):
            assert np.array_equal(sub[k], want["sub_" + k]), (name, "sub-pel", k)


def test_index_tables_are_permutations():
    tables = iu.permutation_tables()
    lengths = {"4x4": 256, "8x8": 64, "16x16": 16, "32x32": 4, "64x64": 1, "8x4": 128, "4x8": 128, "4x16": 64, "16x4": 64, "16x8": 32, "8x16": 32, "32x8": 16,
               "8x32": 16, "32x16": 8, "16x32": 8, "64x16": 4, "16x64": 4, "64x32": 2, "32x64": 2}
    assert set(tables) == set(lengths) and sum(lengths.values()) == iu.N_BLOCKS
    for name, t in tables.items():
        assert len(t) == lengths[name] and sorted(t) == list(range(lengths[name])), name
        inverse = np.argsort(t)
        assert np.array_equal(t[inverse], np.arange(len(t))) and np.array_equal(inverse[t], np.arange(len(t))), name
    assert sorted(iu.PACK_SOURCE) == list(range(iu.N_BLOCKS)) and int(iu.SIDE_4.sum()) == 640
    # every slot's block lies in the superblock, the blocks of a shape tile it
    for w, h, start in iu.SHAPES:
        b = iu.BLOCKS[(iu.BLOCKS[:, 2] == w) & (iu.BLOCKS[:, 3] == h)]
        assert len(b) == 4096 // (w * h) and len({(int(x), int(y)) for x, y, _, _ in b}) == len(b)
        assert (b[:, 0] % w == 0).all() and (b[:, 1] % h == 0).all() and (b[:, 0] + w <= 64).all() and (b[:, 1] + h <= 64).all()
