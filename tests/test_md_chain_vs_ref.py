"""CPU: the restated mode-decision chain (tests/md_chain_util.py: filter search with write-back -> inter and intra prediction into the pool ->
fast cost -> pick -> full loop LUMA -> the CfL service -> full loop CHROMA | DECIDE, each stage fed what the one before it left) against
tests/golden/md_chain.npz, which holds what the reference's own stages made of the same data.  The conditions that make the scenarios
worth chaining are asserted on the restatement's side and again from the fixture's copy of the figures.  Where the reference is present
its drivers are run afresh on the chain's data.  Two mutants of the restated chain -- the write-back dropped, chroma read at p / 2 --
must leave the fixture: a device that got those hand-overs wrong could not pass.  The chain of a size is computed once (well under a
second each) and shared."""
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), ROOT]

import inter_pred_util as ipu  # noqa: E402
import md_chain_util as mc  # noqa: E402
import md_fast_util as mu  # noqa: E402

NAMES = tuple(mc.SIZES)


def test_fixture_holds_the_sizes_of_the_table():
    z = mc.fixture()
    assert tuple(z["sizes"]) == NAMES and mc.CHAIN_SIZES == ("4x16", "8x8", "16x16", "32x8", "64x64")
    assert {n: mc.SIZES[n][2:5] for n in mc.CHAIN_SIZES} == {"4x16": (None, False, "m1"), "8x8": ("fast", True, "m1"), "16x16": ("full", True, "m0"),
                                                            "32x8": ("fast", True, "none"), "64x64": ("fast", False, "m0")}
    assert os.path.getsize(mc.FIXTURE) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "post_filter_chain.npz"))


@pytest.mark.parametrize("name", NAMES)
def test_generated_inputs_are_the_fixtures(name):
    s, want = mc.make_scenario(name), mc.expected(name)
    for k, v in mc.input_digests(s).items():
        assert np.array_equal(v, want["sha256_" + k]), (name, k)
    # the scenario of the issue: the picture, the borders, the blocks, the candidates, the buffers
    w, h = s.w, s.h
    assert s.src[0].shape == (mc.PIC_H, mc.PIC_W) == (64, 128) and s.src[1].shape == (32, 64) and s.ref0.border == s.ref1.border == ipu.border_for(w, h)
    xs, ys = {x for x, _ in s.block_xy}, {y for _, y in s.block_xy}
    assert {(0, 0), (128 - w, 0), (0, 64 - h), (128 - w, 64 - h)} <= set(s.block_xy) and len(set(s.block_xy)) == s.n_groups
    assert {0, 128 - w} <= xs and {0, 64 - h} <= ys
    assert s.n_groups == 2 if name == "64x64" else 12 <= s.n_groups <= 24
    assert all(3 <= int(c) <= 7 for c in s.groups["count"]) and set(s.groups["buffer_width"]) == {13} and s.max_full == 4
    assert set(s.groups["buffer_total_count"].tolist()) - {0} <= {1, 2, 3, 4} and len(set(s.groups["buffer_total_count"].tolist())) >= (2 if s.n_groups == 2 else 4)
    kinds = set(s.kind)
    assert {"DC", "MERGE"} <= kinds and kinds & {"L0f", "L0w"} and kinds & {"L1f", "L1w"} and kinds & {"BI", "BIw"}
    assert s.n_groups == 2 or ({"V", "H", "PAETH", "SMOOTH", "DIR"} <= kinds and {"L0f", "L0w", "L1f", "L1w", "BI"} <= kinds)
    assert any(d for m, d in s.luma_mode if m in range(1, 9))                            # a directional mode with an angle_delta
    n_invalid = int(((s.fast["flags"] & mu.INVALID) != 0).sum())
    assert 1 <= n_invalid <= max(1, (s.n_groups + 2) // 3)
    # the searched candidates are a prefix of the PU descriptors: both sides above 4, no merge candidate
    searched = [min(w, h) > 4 and s.kind[r] != "MERGE" for r in s.pu_row]
    assert searched == [True] * s.n_search + [False] * (len(s.pu) - s.n_search) and (s.n_search > 0) == bool(s.ifs)
    assert not s.ifs or not s.pu["interp_filters"].any()
    # intra blocks without a row above or a column to the left
    d, _ = mc.intra_descs(s, 0, 128, 128, s.pool[0].shape[1], 0)
    assert (d["n_top_px"] == 0).any() and (d["n_left_px"] == 0).any() and (s.n_groups == 2 or ((d["n_top_px"] > 0) & (d["n_left_px"] > 0)).any())
    if w == 4:
        assert {0, 1} <= set(s.fast["has_uv"].tolist()) and any(ipu.sub8x8(p, w, h) for p in s.pu)


@pytest.mark.parametrize("name", NAMES)
def test_restated_chain_equals_the_fixture_at_every_stage(oracle, name):
    s, chain = mc.chain_of(name, oracle)
    want = mc.expected(name)
    assert mc.first_difference(chain, want) is None, (name, mc.first_difference(chain, want))
    assert mc.total_refused(chain) == want["refused"] == (3 if mc.SIZES[name][5] else 0)


@pytest.mark.parametrize("name", NAMES)
def test_scenarios_meet_their_conditions(oracle, name):
    s, chain = mc.chain_of(name, oracle)
    m = mc.measures(s, chain)
    assert m == mc.expected(name)["measures"], name
    ok = mc.conditions(name, m)
    assert all(ok.values()), (name, [k for k, v in ok.items() if not v])
    assert len(ok) == 7 + bool(mc.SIZES[name][2]) + 3 * mc.SIZES[name][3]


def test_reference_drivers_run_afresh_on_the_chain(oracle):
    """the reference's drivers of every stage, built and run now on the chain's data, against the restated chain and the fixture"""
    import make_golden_md_chain as mg
    if not mg.reference_available():
        pytest.skip("the reference and its objects exist in the build container only")
    with tempfile.TemporaryDirectory() as tmp:
        D = mg.Drivers(tmp)
        for name in NAMES:
            ref = mg.reference_chain(D, name, oracle)      # asserts every stage equal to the restated chain's
            assert mc.first_difference(ref, mc.expected(name)) is None, (name, mc.first_difference(ref, mc.expected(name)))


@pytest.mark.parametrize("name", [n for n in mc.CHAIN_SIZES if mc.SIZES[n][2]])
def test_fixture_tells_a_dropped_write_back(oracle, name):
    """the prediction running with interp_filters = 0 instead of the searched filters: the decisions or the reconstructed picture change"""
    _, chain = mc.chain_of(name, oracle, write_back=False)
    want = mc.expected(name)
    assert mc.first_difference(chain, want, only=("ifs",)) is None
    assert mc.first_difference(chain, want, only=("pu",)) is not None and mc.first_difference(chain, want, only=("pool_luma",)) is not None
    assert mc.first_difference(chain, want, only=("decision", "recon")) is not None, name


def test_fixture_tells_chroma_read_at_half_the_position(oracle):
    """4x16: the fast cost and the full loop taking their chroma positions as p / 2 instead of ((p >> 3) << 3) / 2.  Pool tiles sit at a pitch
    of 8 (tw = max(8, w)), so pred_x is a multiple of 8 and both forms give the same pool position: no pool read moves.  What moves, for the
    blocks at x % 8 == 4, is the source position in the fast cost and the full loop, the latter's position in the reconstructed picture, and
    the position the chroma intra edges are read at (md_chain_util.intra_descs).  So the test pins the source-side and recon-side positions, not the pool-side ones; those
    are pinned by the pool's chroma planes themselves, which the prediction entries write and the fixture holds"""
    s0 = mc.make_scenario("4x16")
    assert not (s0.fast["pred_x"] % 8).any() and (s0.fast["src_x"] % 8 == 4).any()
    _, chain = mc.chain_of("4x16", oracle, half_chroma=True)
    want = mc.expected("4x16")
    assert mc.first_difference(chain, want, only=("pu", "pool_luma")) is None
    assert mc.first_difference(chain, want, only=("fast",)) is not None
    assert mc.first_difference(chain, want, only=("decision", "recon")) is not None
