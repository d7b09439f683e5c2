"""Writes tests/golden/fg_denoise.npz from the reference's own film-grain Wiener denoising (tests/golden/ref_fg_denoise_driver.c, linked by the
recipe of oracle/ref_driver.py against the reference objects of the oracle build, oracle/_ref/obj_all).  Run in the build container only,
where the reference exists: the fixture is data.

    python tests/golden/make_golden_fg_denoise.py

Pictures, contents, spectra and cases: fg_denoise_util.PICTURES / CASES; planes and spectra are fg_denoise_util.planes_of / psd_of and are
not stored.  Contents:
  den_<case>_<plane>      the samples aom_wiener_denoise_2d wrote
  result_sha_<case>_<plane>   SHA-256 of the float plane before the dither over the picture area.  The reference keeps that plane to
                          itself: it is the restatement's, whose dither of it is asserted to give the reference's samples, and the tests
                          compare the device's floats with the restatement's own, whose digest they check against this one
  chain_<p>, chain_map_<p>, chain_den_<p>_<plane>   per picture of fg_model_util: the state, final flat-block map and denoised planes of
                          aom_flat_block_finder_run + aom_wiener_denoise_2d + aom_noise_model_update with the default psd at noise level 5.0
The restatement (tests/fg_denoise_util.py) is asserted equal to the reference for every sample while the fixture is written, and the cases
together must reach every key of fg_denoise_util.COVERAGE_KEYS."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "svt-av1-1_amd", "python")]

import fg_denoise_util as du  # noqa: E402
import fg_model_util as mu  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


def build_driver(out_dir):
    """ref_fg_denoise_driver.c by the recipe of oracle/ref_driver.py, with its signatures"""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_fg_denoise_driver.c"), out_dir, include=(os.path.join(ROOT, "include"),))
    V, I, F = C.c_void_p, C.c_int, C.c_float
    L.drv_fgd_denoise.argtypes = [I] * 3 + [V] * 6 + [I] * 3 + [V] * 3
    L.drv_fgd_fft.argtypes = [I, V, V]
    L.drv_fgd_ifft.argtypes = [I, V, V]
    L.drv_fgd_tx.argtypes = [I, V, V]
    L.drv_fgd_extract.argtypes = [I, I, V, I, I, I, I, I, V, V]
    L.drv_fgd_psd.restype = F
    L.drv_fgd_psd.argtypes = [I, F]
    L.drv_fgd_chain.argtypes = [I] * 3 + [V] * 6 + [I] * 3 + [F, V, V]
    L.drv_fgd_time.restype = C.c_double
    L.drv_fgd_time.argtypes = [I] * 4 + [V] * 6 + [I] * 3 + [V] * 3
    return L


def reference_denoise(L, bd, data, psd):
    """the planes aom_wiener_denoise_2d writes"""
    h, w = data[0].shape
    data = [np.ascontiguousarray(a) for a in data]
    den = [np.zeros_like(a) for a in data]
    psd = [np.ascontiguousarray(a, dtype=np.float32) for a in psd]
    assert L.drv_fgd_denoise(bd, w, h, *[a.ctypes.data for a in data], *[a.ctypes.data for a in den], *[a.shape[1] for a in data], *[a.ctypes.data for a in psd]) == 1
    return den


def reference_fft(L, block):
    n = block.shape[0]
    a, out = np.ascontiguousarray(block, dtype=np.float32), np.zeros((n, n, 2), np.float32)
    assert L.drv_fgd_fft(n, a.ctypes.data, out.ctypes.data) == 0
    return out[:, :, 0], out[:, :, 1]


def reference_ifft(L, re, im):
    """re, im [n, n/2 + 1]: the other columns are zero, as aom_noise_tx_malloc leaves them"""
    n = re.shape[0]
    a = np.zeros((n, n, 2), np.float32)
    a[:, :n // 2 + 1, 0], a[:, :n // 2 + 1, 1] = re, im
    out = np.zeros((n, n), np.float32)
    assert L.drv_fgd_ifft(n, a.ctypes.data, out.ctypes.data) == 0
    return out


def reference_tx(L, block, psd):
    a, psd = np.ascontiguousarray(block, dtype=np.float32).copy(), np.ascontiguousarray(psd, dtype=np.float32)
    assert L.drv_fgd_tx(a.shape[0], a.ctypes.data, psd.ctypes.data) == 0
    return a


def reference_block(L, bd, n, plane, offsx, offsy):
    plane = np.ascontiguousarray(plane)
    fit, block = np.zeros(n * n), np.zeros(n * n)
    assert L.drv_fgd_extract(bd, n, plane.ctypes.data, plane.shape[1], plane.shape[0], plane.shape[1], offsx, offsy, fit.ctypes.data, block.ctypes.data) == 0
    return fit, block


def reference_chain(L, bd, data, noise_level):
    """(state, final map, denoised planes) of the three calls of aom_denoise_and_model_run"""
    h, w = data[0].shape
    data = [np.ascontiguousarray(a) for a in data]
    den = [np.zeros_like(a) for a in data]
    nbw, nbh = mu.blocks_of(w, h)
    flat, state = np.zeros(nbw * nbh, np.uint8), np.zeros((), mu.STATE)
    status = L.drv_fgd_chain(bd, w, h, *[a.ctypes.data for a in data], *[a.ctypes.data for a in den], *[a.shape[1] for a in data], noise_level, flat.ctypes.data,
                             state.ctypes.data)
    assert status >= 0 and status == state["status"]
    return state, flat, den


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    out, cov = {}, du.new_coverage()
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for k, (p, content, kind) in enumerate(du.CASES):
            w, h, bd = du.PICTURES[p]
            data, psd = du.planes_of(p, content), du.psd_of(kind, k)
            ref = reference_denoise(L, bd, data, psd)
            planes, mine = du.denoise(data, bd, psd, cov)
            for c in range(3):
                assert np.array_equal(ref[c], mine[c]), ("the restatement differs from the reference", k, c, np.argwhere(ref[c] != mine[c])[:4])
                out[f"den_{k}_{c}"] = ref[c]
                out[f"result_sha_{k}_{c}"] = du.digest(du.picture_area(planes, w, h)[c])
            print("case", k, (w, h, bd), content, kind, "changed samples", [int((ref[c] != data[c]).sum()) for c in range(3)])
        for p in range(len(mu.PICTURES)):
            w, h, bd = mu.PICTURES[p]
            assert du.PICTURES[p] == mu.PICTURES[p]
            data = mu.planes_of(p)[0]
            state, flat, den = reference_chain(L, bd, data, du.NOISE_LEVEL)
            _, mine = du.denoise(data, bd, du.psd_of("default"))
            assert all(np.array_equal(den[c], mine[c]) for c in range(3)), ("chain", p)
            assert np.array_equal(flat, fixture_final(p)), "aom_flat_block_finder_run gives another map than fg_model.npz records"
            got = mu.noise_model(bd, data, den, flat.reshape(mu.blocks_of(w, h)[::-1]))
            assert mu.same_bits(state, got), ("the noise model's restatement differs on the denoised planes", p, mu.differing_fields(state, got))
            out[f"chain_{p}"], out[f"chain_map_{p}"] = np.frombuffer(state.tobytes(), np.uint8), flat
            for c in range(3):
                out[f"chain_den_{p}_{c}"] = den[c]
            print("chain", p, (w, h, bd), "map", flat.tolist(), "status", int(state["status"]))
    print("coverage", cov)
    assert all(cov[k] for k in du.COVERAGE_KEYS), [k for k in du.COVERAGE_KEYS if not cov[k]]
    out["coverage_keys"] = np.array(du.COVERAGE_KEYS, dtype="U40")
    np.savez_compressed(du.FIXTURE, **out)
    print(f"wrote {du.FIXTURE}: {os.path.getsize(du.FIXTURE)} bytes")
    assert os.path.getsize(du.FIXTURE) <= os.path.getsize(mu.FIXTURE)


def fixture_final(p):
    return mu.fixture()[f"final_{p}"]


if __name__ == "__main__":
    main()
