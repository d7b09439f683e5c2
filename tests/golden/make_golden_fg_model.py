"""Writes tests/golden/fg_model.npz from the reference's own film-grain estimation (tests/golden/ref_fg_model_driver.c, linked by the recipe
of oracle/ref_driver.py against the reference objects of the oracle build, oracle/_ref/obj_all).  Run in the build container only, where
the reference exists: the fixture is data.

    python tests/golden/make_golden_fg_model.py

Pictures, maps and cases: fg_model_util.PICTURES / CASES; planes are fg_model_util.planes_of and are not stored.  Contents:
  state_<case>      the svthip_film_grain_noise_state the driver copied out of aom_noise_model_update, as bytes
  tables            A | AtA_inv of aom_flat_block_finder_init
  features_<p>, is_flat_<p>, final_<p>   per picture: the features and the thresholded bytes (the restatement of :624-670 on the blocks
                    the reference's aom_flat_block_finder_extract_block returned, asserted equal to the restatement's own blocks) and the
                    final map of the reference's aom_flat_block_finder_run, which the numpy finish on those features is asserted to give
  chain_<p>         the state of aom_noise_model_update with that final map
The restatement (tests/fg_model_util.py) is asserted equal to the reference bit for bit for every state and block while the fixture is
written, no score may be tied at the decile threshold, and the cases together must reach every key of fg_model_util.COVERAGE_KEYS."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "svt-av1-1_amd", "python")]

import fg_model_util as mu  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


def build_driver(out_dir):
    """ref_fg_model_driver.c by the recipe of oracle/ref_driver.py, with its signatures"""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_fg_model_driver.c"), out_dir, include=(os.path.join(ROOT, "include"),))
    V, I = C.c_void_p, C.c_int
    L.drv_fgm_update.argtypes = [I] * 3 + [V] * 6 + [I] * 3 + [V, V]
    L.drv_fgm_tables.argtypes = [I, V]
    L.drv_fgm_flat_run.argtypes = [I, V, I, I, I, V]
    L.drv_fgm_extract.argtypes = [I, V, I, I, I, I, I, V, V]
    L.drv_fgm_time.restype = C.c_double
    L.drv_fgm_time.argtypes = [I] * 5 + [V] * 6 + [I] * 3 + [V]
    assert L.drv_fgm_state_size() == mu.STATE.itemsize
    return L


def _plane_args(data, den):
    data, den = [np.ascontiguousarray(a) for a in data], [np.ascontiguousarray(a) for a in den]
    return data, den, [a.ctypes.data for a in data] + [a.ctypes.data for a in den] + [a.shape[1] for a in data]


def reference_state(L, bd, data, den, flat):
    """the state after aom_noise_model_init + aom_noise_model_update"""
    h, w = data[0].shape
    keep = _plane_args(data, den)
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    out = np.zeros((), mu.STATE)
    status = L.drv_fgm_update(bd, w, h, *keep[2], flat.ctypes.data, out.ctypes.data)
    assert status >= 0 and status == out["status"]
    return out


def reference_tables(L, bd):
    out = np.zeros(mu.TABLES_DOUBLES)
    assert L.drv_fgm_tables(bd, out.ctypes.data) == 0
    return out


def reference_block(L, bd, luma, offsx, offsy):
    luma = np.ascontiguousarray(luma)
    plane, block = np.zeros(mu.BLOCK ** 2), np.zeros(mu.BLOCK ** 2)
    assert L.drv_fgm_extract(bd, luma.ctypes.data, luma.shape[1], luma.shape[0], luma.shape[1], offsx, offsy, plane.ctypes.data, block.ctypes.data) == 0
    return plane, block


def reference_final_map(L, bd, luma):
    luma = np.ascontiguousarray(luma)
    nbw, nbh = mu.blocks_of(luma.shape[1], luma.shape[0])
    out = np.zeros(nbw * nbh, np.uint8)
    n = L.drv_fgm_flat_run(bd, luma.ctypes.data, luma.shape[1], luma.shape[0], luma.shape[1], out.ctypes.data)
    assert n == np.count_nonzero(out)
    return out


def reference_features(L, bd, luma):
    """the features of :624-670 on the reference's own extracted blocks, each asserted equal to the restatement's block"""
    tables = reference_tables(L, bd)
    h, w = luma.shape
    nbw, nbh = mu.blocks_of(w, h)
    feat, flat = np.zeros(nbw * nbh, mu.FEATURES), np.zeros(nbw * nbh, np.uint8)
    for b in range(nbw * nbh):
        ox, oy = (b % nbw) * mu.BLOCK, (b // nbw) * mu.BLOCK
        plane, block = reference_block(L, bd, luma, ox, oy)
        my_plane, my_block = mu.extract_block(luma, bd, ox, oy, tables)
        assert mu.same_bits(plane, my_plane) and mu.same_bits(block, my_block), ("the restatement's block differs from the reference", (w, h), b)
        (feat[b]["trace"], feat[b]["ratio"], feat[b]["norm"], feat[b]["var"]), flat[b] = mu.block_features(block)
    return feat, flat


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    out, cov = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        tables = reference_tables(L, 8)
        assert mu.same_bits(tables, reference_tables(L, 10)) and mu.same_bits(tables, mu.flat_tables()), "the tables differ from the reference"
        out["tables"] = tables
        for k, (p, kind, variant) in enumerate(mu.CASES):
            w, h, bd = mu.PICTURES[p]
            data, den = mu.planes_of(p, variant)
            flat = mu.flat_map(p, kind)
            ref = reference_state(L, bd, data, den, flat)
            mine = mu.noise_model(bd, data, den, flat, cov)
            assert mu.same_bits(ref, mine), ("the restatement differs from the reference", k, mu.differing_fields(ref, mine))
            assert not any(np.isnan(ref[s][c][f]).any() for s in ("latest", "combined") for c in range(3) for f in ref[s].dtype.names)
            out[f"state_{k}"] = np.frombuffer(ref.tobytes(), np.uint8)
            print("case", k, (w, h, bd), kind, variant, "status", int(ref["status"]), "observations", ref["latest"]["num_observations"].tolist(),
                  "equations", ref["latest"]["strength_num_equations"].tolist())
        for p, (w, h, bd) in enumerate(mu.PICTURES):
            data, den = mu.planes_of(p)
            feat, is_flat = reference_features(L, bd, data[0])
            mine = mu.flat_block_features(data[0], bd)
            assert mu.same_bits(feat, mine[0]) and mu.same_bits(is_flat, mine[1])
            assert not any(np.isnan(feat[f]).any() for f in feat.dtype.names)
            final = reference_final_map(L, bd, data[0])
            got, scores, threshold = mu.finish_flat_blocks(feat, is_flat)
            assert (scores == threshold).sum() == 1, ("scores are tied at the decile threshold", p, scores)
            assert np.array_equal(got, final), ("the numpy finish differs from aom_flat_block_finder_run", p, got, final)
            chain = reference_state(L, bd, data, den, final.reshape(mu.blocks_of(w, h)[::-1]))
            assert mu.same_bits(chain, mu.noise_model(bd, data, den, final.reshape(mu.blocks_of(w, h)[::-1]), cov))
            out[f"features_{p}"], out[f"is_flat_{p}"], out[f"final_{p}"] = np.frombuffer(feat.tobytes(), np.uint8), is_flat, final
            out[f"chain_{p}"] = np.frombuffer(chain.tobytes(), np.uint8)
            print("picture", p, (w, h, bd), "is_flat", is_flat.tolist(), "final", final.tolist(), "chain status", int(chain["status"]))
    print("coverage", {k: bool(cov.get(k)) for k in mu.COVERAGE_KEYS})
    assert all(cov.get(k) for k in mu.COVERAGE_KEYS), [k for k in mu.COVERAGE_KEYS if not cov.get(k)]
    out["coverage_keys"] = np.array(mu.COVERAGE_KEYS, dtype="U40")
    np.savez_compressed(mu.FIXTURE, **out)
    print(f"wrote {mu.FIXTURE}: {os.path.getsize(mu.FIXTURE)} bytes")
    assert os.path.getsize(mu.FIXTURE) <= 1_000_000


if __name__ == "__main__":
    main()
