"""CPU: the restated chain deblocking pick -> deblocking -> CDEF search and pick for 128-wide blocks -> CDEF frame filter
(tests/post_filter_chain128_util.py) against tests/golden/post_filter_chain128.npz, which holds what the reference's own stages made of
the same two pictures as a chain.  Where the reference is present the chain of the 10-bit picture is run afresh."""
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), ROOT]

import cdef128_util as c128  # noqa: E402
import dlf_util as du  # noqa: E402
import post_filter_chain128_util as pc128  # noqa: E402
import post_filter_chain_util as pc  # noqa: E402

NAMES = tuple(pc128.PICTURES)
_cache = {}


def restated(name):
    if name not in _cache:
        _cache[name] = pc128.chain_of(name)
    return _cache[name]


@pytest.mark.parametrize("name", NAMES)
def test_pictures_are_the_fixtures_and_have_the_layout_of_case_b(name):
    mi, recon, source, _ = restated(name)
    want = pc128.expected(name)
    assert tuple(pc128.fixture()["pictures"]) == NAMES and [pc128.PICTURES[n]["bd"] for n in NAMES] == [8, 10]
    for k, v in pc.input_digests(mi, recon, source).items():
        assert np.array_equal(v, want["sha256_" + k]), (name, k)
    skip, sb = pc128.grids(mi)
    assert np.array_equal(sb, c128.make_grid("B", pc128.W, pc128.H))
    wide = np.isin(mi["sb_type"], (c128.BLOCK_128X128, c128.BLOCK_128X64, c128.BLOCK_64X128))
    assert (mi["tx_size"][wide] == du.TX_OF[(64, 64)]).all() and wide.any()
    # chroma of a wide block: 64 samples of the plane each way, the transform the deblocking rule derives 32x32
    txw, txh, bw, bh, _ = du.plane_geometry(mi, 1)
    assert (txw[wide[1::2, 1::2]] == 32).all() and (txh[wide[1::2, 1::2]] == 32).all()


@pytest.mark.parametrize("name", NAMES)
def test_restated_chain_equals_the_fixture_at_every_stage(name):
    _, recon, _, chain = restated(name)
    want = pc128.expected(name, recon)
    assert pc128.first_difference(chain, want) is None, (name, pc128.first_difference(chain, want))
    for k in pc128.PLANE_STAGES:
        assert pc.plane_digest(chain[k])[0] == want["digest_" + k][0], (name, k)
    ok = pc128.conditions(recon, chain)
    assert all(ok.values()), (name, [k for k, v in ok.items() if not v])


def test_reference_chain_run_afresh():
    import make_golden_post_filter_chain128 as mg
    if not mg.reference_available():
        pytest.skip("the reference and its objects exist in the build container only")
    name = "B"
    P = pc128.PICTURES[name]
    mi, recon, source, chain = restated(name)
    with tempfile.TemporaryDirectory() as tmp:
        ref = mg.reference_chain(mg.Drivers(tmp), recon, source, mi, P["bd"], P["last_levels"], P["base_qindex"])
    assert pc128.first_difference(chain, ref) is None, pc128.first_difference(chain, ref)
    assert pc128.first_difference(ref, pc128.expected(name, recon)) is None
