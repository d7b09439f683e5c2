"""CPU: the restatement of film-grain synthesis (tests/film_grain_util.py) against the reference's av1_add_film_grain_run -- against the
recorded fixture (tests/golden/film_grain.npz) everywhere, and against the live driver (tests/golden/ref_film_grain_driver.c) where the
reference is available; the Gaussian table and its generated .inc; the parameter block's layout against the header and, where the
reference is present, the header's against aom_film_grain_t.  Parameter sets with num_y_points == 0 (film_grain_util.REFERENCE_UNSAFE)
are never given to the reference: its dealloc_arrays frees one pointer more than init_arrays allocated."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")]

import film_grain_util as fu  # noqa: E402
import gen_film_grain_gauss as gauss  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

KEYS = "y cb cr".split()


def test_fixture_has_the_cases():
    fx = fu.fixture()
    assert os.path.getsize(fu.FIXTURE) <= 450_000
    assert [tuple(int(v) for v in c) for c in fx["sizes"]] == list(fu.SIZES) and tuple(int(v) for v in fx["big"]) == fu.BIG
    assert np.array_equal(fx["params"], np.stack([np.frombuffer(fu.pack_params(p), np.uint8) for p in fu.PARAM_SETS]))
    assert 8 <= len(fu.PARAM_SETS) <= 12 and fu.REFERENCE_UNSAFE
    for s, bd, z in fu.all_cases():
        i = fu.BIT_DEPTHS.index(bd)
        if s in fu.REFERENCE_UNSAFE:
            assert fx["digest"][z, s, i] == 0 and f"tables_s{s}_b{bd}" not in fx
        else:
            assert fx["digest"][z, s, i] != 0 and fx[f"tables_s{s}_b{bd}"].shape == (fu.TABLES_INT16,)
    for z, combos in fu.KEPT.items():
        for s, bd in combos:
            w, h = fu.SIZES[z]
            assert fx[f"out_z{z}_s{s}_b{bd}_y"].shape == (h, w) and fx[f"out_z{z}_s{s}_b{bd}_cb"].shape == (h // 2, w // 2)
    assert {bd for _, _, bd in fu.AV1_WRAPPER} == {8, 10} and all(f"out_z{z}_s{s}_b{bd}_y" in fx for z, s, bd in fu.AV1_WRAPPER)


@pytest.mark.parametrize("bd", fu.BIT_DEPTHS)
@pytest.mark.parametrize("s", range(len(fu.PARAM_SETS)))
def test_restatement_matches_fixture(s, bd):
    fx = fu.fixture()
    p, t = fu.PARAM_SETS[s], fu.tables_of(s, bd)
    if s in fu.REFERENCE_UNSAFE:
        assert not t["luma"].any() and t["cb"].any() and t["cr"].any()
        return
    assert np.array_equal(fu.tables_block(t), fx[f"tables_s{s}_b{bd}"])
    for z, (w, h) in enumerate(fu.SIZES):
        planes = fu.source_planes(w, h, bd, s)
        mine = fu.add_film_grain(p, bd, *planes, t=t)
        assert fu.digest(mine) == fx["digest"][z, s, fu.BIT_DEPTHS.index(bd)], ((w, h), s, bd)
        if f"out_z{z}_s{s}_b{bd}_y" in fx:
            for k, a in zip(KEYS, mine):
                assert a.dtype == fx[f"out_z{z}_s{s}_b{bd}_{k}"].dtype and np.array_equal(a, fx[f"out_z{z}_s{s}_b{bd}_{k}"]), ((w, h), s, bd, k)


def test_restatement_matches_fixture_at_1080p():
    fx = fu.fixture()
    w, h = fu.BIG
    mine = fu.add_film_grain(fu.PARAM_SETS[fu.BIG_SET], 8, *fu.source_planes(w, h, 8, fu.BIG_SET), t=fu.tables_of(fu.BIG_SET, 8))
    assert fu.digest(mine) == fx["digest"][len(fu.SIZES), fu.BIG_SET, 0]


def test_planes_without_points_are_copied():
    for s, p in enumerate(fu.PARAM_SETS):
        planes = fu.source_planes(72, 40, 8, s)
        out = fu.add_film_grain(p, 8, *planes, t=fu.tables_of(s, 8))
        for k, n in enumerate((p["num_y_points"], p["num_cb_points"], p["num_cr_points"])):
            assert n > 0 or np.array_equal(out[k], planes[k]), (s, k)


def test_fixture_covers_the_ground():
    fx = fu.fixture()
    assert tuple(fx["coverage_keys"]) == fu.COVERAGE_KEYS
    cov = fu.coverage([(fu.PARAM_SETS[s], bd, *fu.size_of(z)) for s, bd, z in fu.all_cases() if z < len(fu.SIZES)])
    assert all(cov.values()), [k for k, v in cov.items() if not v]


def test_gaussian_table():
    assert len(gauss.GAUSS) == 2048 and all(v % 4 == 0 and -2048 <= v <= 2047 for v in gauss.GAUSS)
    assert abs(sum(gauss.GAUSS)) < 2048 * 16 and 480 < np.std(gauss.GAUSS) < 540
    with open(os.path.join(ROOT, "svt-av1-1_amd", "csrc", "av1_film_grain_gauss.inc")) as f:
        assert f.read() == gauss.render(), "run tools/gen_film_grain_gauss.py"
    # every entry is pinned through the reference's own templates: at lag 0, 10 bits and grain_scale_shift 0 a template sample is entry / 4
    fx = fu.fixture()
    seen = np.zeros(2048, bool)
    quarters = np.array(gauss.QUARTERS)
    for s, p in enumerate(fu.PARAM_SETS):
        if p["ar_coeff_lag"] == 0 and p["grain_scale_shift"] == 0 and s not in fu.REFERENCE_UNSAFE and p["ar_coeffs_cb"][0] == p["ar_coeffs_cr"][0] == 0:
            t = fu.split_block(fx[f"tables_s{s}_b10"])
            for name, row, n in (("luma", None, fu.LUMA_H * fu.LUMA_W), ("cb", 7, fu.CHROMA_H * fu.CHROMA_W), ("cr", 11, fu.CHROMA_H * fu.CHROMA_W)):
                idx, _ = fu._draws(p["random_seed"] if row is None else fu.row_seed(p["random_seed"], row), n, 11)
                assert np.array_equal(t[name].reshape(-1), quarters[idx]), (s, name)
                seen[idx] = True
    assert seen.all()


def test_parameter_block_layout_equals_the_headers():
    import svtav1_hip
    from svtav1_hip import _abi
    offs = svtav1_hip.film_grain_param_offsets()
    assert svtav1_hip.FILM_GRAIN_PARAMS_BYTES == fu.PARAMS_BYTES and list(offs)[:-2] == [n for n, _ in fu.FIELDS]
    assert svtav1_hip.FILM_GRAIN_TABLES_BYTES == 2 * (_abi.define("SVTHIP_FILM_GRAIN_LUMA_H") * _abi.define("SVTHIP_FILM_GRAIN_LUMA_W") + 2 *
                                                      _abi.define("SVTHIP_FILM_GRAIN_CHROMA_H") * _abi.define("SVTHIP_FILM_GRAIN_CHROMA_W") + 768)
    assert [_abi.define("SVTHIP_FILM_GRAIN_" + k) for k in ("LUMA_H", "LUMA_W", "CHROMA_H", "CHROMA_W")] == [fu.LUMA_H, fu.LUMA_W, fu.CHROMA_H, fu.CHROMA_W]
    layout = _abi.dtype("svthip_film_grain_params")
    assert svtav1_hip.FILM_GRAIN_PARAMS_BYTES == layout.itemsize and offs == {k: layout.fields[k][1] for k in layout.names}
    # the packer and the test utility's independent packer agree byte for byte
    for p in fu.PARAM_SETS:
        assert bytes(svtav1_hip.film_grain_params(**p)) == fu.pack_params(p)
    assert fu.TABLES_INT16 * 2 == svtav1_hip.FILM_GRAIN_TABLES_BYTES
    with pytest.raises(TypeError):
        svtav1_hip.film_grain_params(no_such_field=1)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not reference_available():
        pytest.skip("the reference sources and oracle/_ref/obj_all are not here")
    import make_golden_film_grain as gen
    return gen, gen.build_driver(str(tmp_path_factory.mktemp("film_grain_ref")))


def test_headers_struct_is_the_references(driver):
    import svtav1_hip
    gen, L = driver
    offs = svtav1_hip.film_grain_param_offsets()
    ref = np.zeros(32, np.int32)
    n = L.drv_fg_params_offsets(ref.ctypes.data)
    assert L.drv_fg_params_size() == svtav1_hip.FILM_GRAIN_PARAMS_BYTES
    assert list(ref[:n]) == [o for k, o in offs.items() if k != "reserved"]


def test_restatement_matches_live_reference(driver):
    gen, L = driver
    fx = fu.fixture()
    for s, p in enumerate(fu.PARAM_SETS):
        if s in fu.REFERENCE_UNSAFE:
            continue        # never: see the module docstring
        for bd in fu.BIT_DEPTHS:
            ref = gen.reference_tables(L, p, bd)
            assert np.array_equal(fu.tables_block(fu.tables_of(s, bd)), ref) and np.array_equal(fx[f"tables_s{s}_b{bd}"], ref), (s, bd)
            for z, (w, h) in enumerate(fu.SIZES):
                planes = fu.source_planes(w, h, bd, s)
                out = gen.reference_run(L, p, bd, planes, wrapper=(z, s, bd) in fu.AV1_WRAPPER)
                mine = fu.add_film_grain(p, bd, *planes, t=fu.tables_of(s, bd))
                for k, a, b in zip(KEYS, mine, out):
                    assert np.array_equal(a, b), ((w, h), s, bd, k)
                assert fu.digest(out) == fx["digest"][z, s, fu.BIT_DEPTHS.index(bd)]
