"""CPU: the restated post-reconstruction chain (tests/post_filter_chain_util.py: deblocking pick -> deblocking -> CDEF search, pick and
frame -> Wiener and self-guided searches -> restoration -> film grain, each stage fed what the one before it left) against
tests/golden/post_filter_chain.npz, which holds what the reference's own stages made of the same three pictures as a chain.  The
conditions that make the pictures worth chaining are asserted on the restatement's side.  Where the reference is present its chain of
one picture is run afresh.  The chain of a picture is computed once per module (about 4 s each)."""
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), ROOT]

import cdef_util as cu  # noqa: E402
import lr_util as lu  # noqa: E402
import post_filter_chain_util as pc  # noqa: E402

NAMES = tuple(pc.PICTURES)
_cache = {}


def restated(name):
    """(mi, recon, source, chain): shared by the tests of this module and left unchanged by them"""
    if name not in _cache:
        _cache[name] = pc.chain_of(name)
    return _cache[name]


def test_fixture_holds_the_pictures_of_the_table():
    z = pc.fixture()
    assert tuple(z["pictures"]) == NAMES == ("A", "B", "C") and tuple(z["whole"]) == ("A",)
    for name, P in pc.PICTURES.items():
        want = pc.expected(name)
        assert all(want[k] == P[k] for k in pc.PARAM_KEYS) and want["last_levels"] == P["last_levels"], name
    assert pc.PICTURES["B"]["base_qindex"] >= 128 and 3 + (pc.PICTURES["B"]["base_qindex"] >> 6) in (5, 6)
    assert pc.PICTURES["A"]["bd"] == 8 and pc.PICTURES["B"]["bd"] == 10
    assert os.path.getsize(pc.FIXTURE) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "lr.npz"))


@pytest.mark.parametrize("name", NAMES)
def test_generated_inputs_are_the_fixtures(name):
    mi, recon, source, _ = restated(name)
    want = pc.expected(name)
    assert mi.shape == (64, 64) and recon[0].shape == (pc.H, pc.W) and recon[1].shape == (pc.H // 2, pc.W // 2)
    for k, v in pc.input_digests(mi, recon, source).items():
        assert np.array_equal(v, want["sha256_" + k]), (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_restated_chain_equals_the_fixture_at_every_stage(name):
    _, recon, _, chain = restated(name)
    want = pc.expected(name, recon)
    assert all((k in want) == (name == "A") for k in pc.PLANE_STAGES)
    assert pc.first_difference(chain, want) is None, (name, pc.first_difference(chain, want))
    for k in pc.PLANE_STAGES:      # the digests of the picture kept whole, too
        assert pc.plane_digest(chain[k])[0] == want["digest_" + k][0], (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_pictures_meet_their_conditions(name):
    _, recon, _, chain = restated(name)
    ok = pc.conditions(name, recon, chain)
    assert all(ok.values()), (name, [k for k, v in ok.items() if not v])
    assert len(ok) == (3 if name == "C" else 9)
    assert not chain["rejected"].any(), "a rejected Wiener unit has no taps to filter with"
    # the geometry the pictures were chosen for
    assert cu.geometry(pc.W, pc.H) == (4, 4) and pc.W % 64 == 8 and pc.H % 64 == 8
    planes, base = lu.picture_units(pc.W, pc.H)
    assert lu.unit_sizes(pc.W, pc.H) == (128, 64, 64) and base == [0, 4, 8, 12] and all(pl[1] == 2 for pl in planes)
    kinds = {(bool(a), bool(b)) for p in range(3) for (_, _, v0, v1) in planes[p][0] for (_, _, a, b) in lu.stripes(int(v0), int(v1), pc.H >> (p > 0), int(p > 0))}
    assert kinds == {(False, True), (True, True), (True, False)}, kinds


def test_reference_chain_run_afresh():
    """the reference's own stages of picture B as a chain, built and run now, against the restated chain and the fixture"""
    import make_golden_post_filter_chain as mg
    if not mg.reference_available():
        pytest.skip("the reference and its objects exist in the build container only")
    name = "B"
    P = pc.PICTURES[name]
    mi, recon, source, chain = restated(name)
    with tempfile.TemporaryDirectory() as tmp:
        ref = mg.reference_chain(mg.Drivers(tmp), recon, source, mi, P["bd"], P["last_levels"], P["base_qindex"], P["grain_set"])
    assert pc.first_difference(chain, ref) is None, pc.first_difference(chain, ref)
    assert pc.first_difference(ref, pc.expected(name)) is None, pc.first_difference(ref, pc.expected(name))
    assert not ref["rejected"].any()
