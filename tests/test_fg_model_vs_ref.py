"""CPU: the restatement of film-grain estimation (tests/fg_model_util.py) against the reference's aom_noise_model_update and flat-block
finder -- against the recorded fixture (tests/golden/fg_model.npz) everywhere, and against the live driver
(tests/golden/ref_fg_model_driver.c) where the reference is available, bit for bit, states, tables, blocks and features; and numpy's finish
of the flat-block finder (score, sort, union) against the reference's final map on every picture of the fixture."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import fg_model_util as mu  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


def _state(raw):
    return np.frombuffer(raw.tobytes(), mu.STATE)[0]


def test_fixture_has_the_cases():
    fx = mu.fixture()
    assert os.path.getsize(mu.FIXTURE) <= 1_000_000
    assert tuple(fx["coverage_keys"]) == mu.COVERAGE_KEYS and fx["tables"].shape == (mu.TABLES_DOUBLES,)
    statuses = [int(_state(fx[f"state_{k}"])["status"]) for k in range(len(mu.CASES))]
    assert {mu.OK, mu.INSUFFICIENT, mu.INTERNAL} == set(statuses)
    assert {mu.PICTURES[p][2] for p, _, _ in mu.CASES} == {8, 10} and (100, 72, 8) in mu.PICTURES and (64, 64, 8) in mu.PICTURES and (96, 40, 10) in mu.PICTURES
    assert {kind for _, kind, _ in mu.CASES} == {"all", "checker", "row", "mixed", "one"} and {v for _, _, v in mu.CASES} == {"noisy", "luma_equal", "chroma_equal"}
    mixed = mu.flat_map(1, "mixed")
    assert {0, 1, 255} == set(mixed.ravel().tolist())
    for p, (w, h, _) in enumerate(mu.PICTURES):
        nb = int(np.prod(mu.blocks_of(w, h)))
        assert fx[f"features_{p}"].size == nb * mu.FEATURES.itemsize and fx[f"is_flat_{p}"].shape == fx[f"final_{p}"].shape == (nb,)
        assert int(_state(fx[f"chain_{p}"])["status"]) == mu.OK


@pytest.mark.parametrize("k", range(len(mu.CASES)))
def test_restatement_matches_fixture(k):
    fx = mu.fixture()
    p, kind, variant = mu.CASES[k]
    data, den = mu.planes_of(p, variant)
    mine = mu.noise_model(mu.PICTURES[p][2], data, den, mu.flat_map(p, kind))
    want = _state(fx[f"state_{k}"])
    assert mine.tobytes() == want.tobytes(), (k, mu.differing_fields(mine, np.asarray(want)))


def test_cases_cover_the_ground():
    cov = {}
    for p, kind, variant in mu.CASES:
        data, den = mu.planes_of(p, variant)
        mu.noise_model(mu.PICTURES[p][2], data, den, mu.flat_map(p, kind), cov)
    assert all(cov.get(k) for k in mu.COVERAGE_KEYS), [k for k in mu.COVERAGE_KEYS if not cov.get(k)]


def test_what_the_states_hold_behind_a_status():
    fx = mu.fixture()
    zero = np.zeros((), mu.STATE)
    for which in ("latest", "combined"):
        zero[which]["ar_gain"] = 1.0
    few = _state(fx["state_2"])            # one flat block: the model as aom_noise_model_init leaves it
    zero["status"] = mu.INSUFFICIENT
    assert few.tobytes() == zero.tobytes()
    failed = _state(fx["state_3"])         # data == denoised on luma: luma's sums are written, nothing behind them
    assert failed["status"] == mu.INTERNAL and failed["latest"][0]["num_observations"] == 3538 and not failed["latest"][0]["A"].any()
    assert not failed["latest"][1]["num_observations"] and failed["combined"].tobytes() == zero["combined"].tobytes()
    fallback = _state(fx["state_4"])       # data == denoised on chroma: only the luma term of A is there, x is the fallback's
    assert fallback["status"] == mu.OK and fallback["latest"][1]["A"][624] > 0 and not fallback["latest"][1]["A"][:624].any()
    assert not fallback["latest"][1]["x"].any()
    ok = _state(fx["state_5"])             # mean / 8192 went into b once for latest and twice for combined
    assert not np.array_equal(ok["latest"][0]["strength_b"], ok["combined"][0]["strength_b"])
    assert np.array_equal(ok["latest"][0]["A"], ok["combined"][0]["A"]) and np.array_equal(ok["latest"][0]["x"], ok["combined"][0]["x"])
    A = ok["latest"][1]["A"][:625].reshape(25, 25)
    assert np.array_equal(A, A.T)


def test_flat_block_features_and_numpy_finish_match_fixture():
    fx = mu.fixture()
    tables = mu.flat_tables()
    assert mu.same_bits(tables, fx["tables"])
    for p, (w, h, bd) in enumerate(mu.PICTURES):     # no picture is left out
        data, _ = mu.planes_of(p)
        feat, is_flat = mu.flat_block_features(data[0], bd, tables)
        assert feat.tobytes() == fx[f"features_{p}"].tobytes() and np.array_equal(is_flat, fx[f"is_flat_{p}"]), p
        final, scores, threshold = mu.finish_flat_blocks(feat, is_flat)
        assert (scores == threshold).sum() == 1, ("scores are tied at the decile threshold", p)
        assert np.array_equal(final, fx[f"final_{p}"]), p
        chain = mu.noise_model(bd, data, mu.planes_of(p)[1], final.reshape(mu.blocks_of(w, h)[::-1]))
        assert chain.tobytes() == fx[f"chain_{p}"].tobytes(), p


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not reference_available():
        pytest.skip("the reference sources and oracle/_ref/obj_all are not here")
    import make_golden_fg_model as gen
    return gen, gen.build_driver(str(tmp_path_factory.mktemp("fg_model_ref")))


def test_restatement_matches_live_reference(driver):
    gen, L = driver
    fx = mu.fixture()
    assert mu.same_bits(gen.reference_tables(L, 8), fx["tables"]) and mu.same_bits(gen.reference_tables(L, 10), fx["tables"])
    for k, (p, kind, variant) in enumerate(mu.CASES):
        data, den = mu.planes_of(p, variant)
        flat = mu.flat_map(p, kind)
        ref = gen.reference_state(L, mu.PICTURES[p][2], data, den, flat)
        assert ref.tobytes() == fx[f"state_{k}"].tobytes(), k
        assert mu.noise_model(mu.PICTURES[p][2], data, den, flat).tobytes() == ref.tobytes(), k
    for p, (w, h, bd) in enumerate(mu.PICTURES):
        data, den = mu.planes_of(p)
        feat, is_flat = gen.reference_features(L, bd, data[0])      # asserts every extracted block equal to the restatement's
        assert feat.tobytes() == fx[f"features_{p}"].tobytes() and np.array_equal(is_flat, fx[f"is_flat_{p}"])
        final = gen.reference_final_map(L, bd, data[0])
        assert np.array_equal(final, fx[f"final_{p}"]) and np.array_equal(mu.finish_flat_blocks(feat, is_flat)[0], final)
        assert gen.reference_state(L, bd, data, den, final.reshape(mu.blocks_of(w, h)[::-1])).tobytes() == fx[f"chain_{p}"].tobytes()
