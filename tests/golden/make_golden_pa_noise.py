"""Writes tests/golden/pa_noise.npz from the reference's own FullSampleDenoise (tests/golden/ref_pa_noise_driver.c, linked by the recipe of
oracle/ref_driver.py against the reference objects of the oracle build, oracle/_ref/obj_all).  Run in the build container only, where the
reference exists: the fixture is data.

    python tests/golden/make_golden_pa_noise.py

Cases (tests/pa_noise_util.py CASES): 64x64 (one SB, picture borders on all four sides), 136x72 and 72x136 (a right column 8 wide, a bottom
row 8 high), 192x192 (a centre SB whose halo comes from all four neighbours), 200x136, 136x728 (height above 720: noiseTh = 0).  Pictures are
constructed and low in entropy, see make_pictures; their chroma is pa_noise_util.chroma_of(luma) and is not stored.  Contents:
  case [6][2]                     width, height
  c{c}_n                          pictures of case c
  c{c}_p{i}_luma                  the unpadded luma of picture i
  c{c}_p{i}_denoised              the reference's denoised luma after DetectInputPictureNoise (the same at both precisions: asserted)
  c{c}_p{i}_den_cb / _den_cr      the reference's Cb and Cr after DenoiseInputPicture, for pictures that take its whole-picture arm
  c{c}_p{i}_s{sub}_sb_var         [n_sb][2] u64: noise variance (raw 16.16) and denoised variance >> 16 of complete SBs, 0 elsewhere
  c{c}_p{i}_s{sub}_flat_noise     [n_sb] u8 sb_flat_noise_array
  c{c}_p{i}_s{sub}_picture        [4] u32: sum of noise variance >> 16, complete SBs, pic_noise_class, picNoiseVarianceFloat >= 1.0
  coverage_keys                   pa_noise_util.COVERAGE_KEYS, all reached: asserted here and by tests/test_pa_noise_vs_ref.py
The reference is run with ASM_AVX2 (as the encoder) and with the C function pointers (ASM_NON_AVX2), with denoiseFlag 0 and 1; both paths
and both flags are asserted to agree on everything copied out, and the restatement (tests/pa_noise_util.py) is asserted equal to them.  The
three planes after DenoiseInputPicture are asserted to be what pa_noise_util._assemble makes of the stored pieces, so they are not stored."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import pa_noise_util as nu  # noqa: E402
import pa_stats_util as pu  # noqa: E402
from make_golden_cdef import save  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


def build_driver(out_dir):
    """ref_pa_noise_driver.c by the recipe of oracle/ref_driver.py, with its signatures"""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_pa_noise_driver.c"), out_dir)
    V = C.c_void_p
    L.drv_pa_noise_open.argtypes = [C.c_int, C.c_int, V, V, V]
    L.drv_pa_noise_run.argtypes = [C.c_int, C.c_int, C.c_int] + [V] * 6
    L.drv_pa_noise_sb_var.argtypes = [C.c_int, C.c_int, V]
    L.drv_pa_noise_time.restype = C.c_double
    L.drv_pa_noise_time.argtypes = [C.c_int, C.c_int]
    return L


def reference_noise(L, luma, cb, cr):
    """{sub: outputs} of one picture from the driver: FIXTURE_OUTPUTS of pa_noise_util.  Runs both asm types and both denoise flags and asserts
    that they agree"""
    h, w = luma.shape
    keep = [np.ascontiguousarray(p, np.uint8) for p in (luma, cb, cr)]
    n_sb = L.drv_pa_noise_open(w, h, *[p.ctypes.data for p in keep])
    assert n_sb == pu.sb_grid(w, h)[0] * pu.sb_grid(w, h)[1]
    outs = {}
    for sub in (0, 1):
        runs = []
        for avx2 in (1, 0):
            for flag in (1, 0):
                o = {"flat_noise": np.zeros(n_sb, np.uint8), "picture": np.zeros(4, np.uint32), "denoised": np.zeros((h, w), np.uint8),
                     "out_luma": np.zeros((h, w), np.uint8), "out_cb": np.zeros((h // 2, w // 2), np.uint8), "out_cr": np.zeros((h // 2, w // 2), np.uint8)}
                rc = L.drv_pa_noise_run(sub, flag, avx2, *[o[k].ctypes.data for k in ("flat_noise", "picture", "denoised", "out_luma", "out_cb", "out_cr")])
                assert rc == 0, ("the reference wrote into the border of the input picture" if rc == -2 else rc)
                o["sb_var"] = np.zeros((n_sb, 2), np.uint64)
                assert L.drv_pa_noise_sb_var(sub, avx2, o["sb_var"].ctypes.data) == 0
                if not flag:   # detection only leaves the input picture alone
                    assert np.array_equal(o["out_luma"], luma) and np.array_equal(o["out_cb"], cb) and np.array_equal(o["out_cr"], cr)
                runs.append((avx2, flag, o))
        first = runs[0][2]
        for avx2, flag, o in runs[1:]:
            for k in first:
                if flag or not k.startswith("out_"):
                    assert np.array_equal(o[k], first[k]), ("ASM_AVX2 and the C path, or the two denoise flags, disagree", (w, h), sub, avx2, flag, k)
        outs[sub] = first
    L.drv_pa_noise_close()
    return outs


def _noisy(base, tile, a):
    h, w = base.shape
    t = np.tile(tile, ((h + 31) // 32, (w + 31) // 32))[:h, :w]
    return np.clip(base.astype(np.int32) + np.rint(a * t).astype(np.int32), 0, 255).astype(np.uint8)


def _tune(make, lo, hi):
    """the first amplitude (steps of 1/16) at which the picture's average noise variance lies in [lo, hi] in the reference's default precision
    (BLOCK_MEAN_PREC_SUB); found with the restatement, which the reference then has to confirm"""
    for a in np.arange(0.25, 80, 0.0625):
        p = make(a)
        total, count = (int(v) for v in nu.detect(p, 1)["picture"][:2])
        if lo <= total // count <= hi:
            return p, float(a)
    raise AssertionError(("no amplitude reaches", lo, hi))


def make_pictures(rng, w, h):
    """[(name, luma)]: a horizontal ramp (no noise to speak of: sum < count, nothing denoised); a picture whose even SBs are flat with mild noise
    (flat = 1) and whose odd SBs carry the same noise on a triangle wave (flat = 0), class 1 with sum >= count: only the flat SBs are denoised; four
    pictures of one 32x32 noise tile on flat 128, the amplitude tuned so that the class is 2, 3, 3_1 and, before the clamp, 4 or more"""
    y, x = np.mgrid[0:h, 0:w]
    tile = rng.uniform(-1, 1, (32, 32))
    flat = np.full((h, w), 128, np.uint8)
    odd_sb = (((x >> 6) + (y >> 6)) & 1) == 1
    mixed = np.where(odd_sb, 64 + np.abs(((x * 4 + y * 2) & 255) - 128), 128).astype(np.uint8)
    th = 25 if h <= 720 else 0
    bands = (("class_2", 5, 9), ("class_3", 10, 16), ("class_3_1", 17, 19), ("clamped", 22, 30))
    pics = [("ramp", (x * 255 // (w - 1)).astype(np.uint8)), ("mixed",) + _tune(lambda a: _noisy(mixed, tile, a), 2, 4)]
    for name, lo, hi in bands:
        pics.append((name,) + _tune(lambda a: _noisy(flat, tile, a), lo + th, hi + th))
    return [(p[0], p[1]) for p in pics]


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    rng = np.random.default_rng(20261019)
    out = {"case": np.array(nu.CASES, np.int32)}
    seen = []
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for c, (w, h) in enumerate(nu.CASES):
            pics = make_pictures(rng, w, h)
            out[f"c{c}_n"] = np.int32(len(pics))
            for i, (name, luma) in enumerate(pics):
                cb, cr = nu.chroma_of(luma)
                ref = reference_noise(L, luma, cb, cr)
                assert np.array_equal(ref[0]["denoised"], ref[1]["denoised"])
                out[f"c{c}_p{i}_luma"], out[f"c{c}_p{i}_denoised"] = luma, ref[0]["denoised"]
                for sub in (0, 1):
                    r = ref[sub]
                    mine = nu.detect(luma, sub)
                    for k in nu.DETECT_OUTPUTS + ("denoised",):
                        assert np.array_equal(mine[k], r[k]), ("the restatement differs from the reference", (w, h), name, sub, k, mine[k], r[k])
                    planes = nu.denoise(luma, cb, cr, mine)
                    whole = nu.arm(r["picture"]) == "whole_picture"
                    pieces = nu._assemble(luma, cb, cr, r, r["out_cb"] if whole else None, r["out_cr"] if whole else None)
                    for k, p, q in zip(("out_luma", "out_cb", "out_cr"), planes, pieces):
                        assert np.array_equal(p, r[k]) and np.array_equal(q, r[k]), ("the restatement differs from the reference", (w, h), name, sub, k)
                    if whole:
                        out[f"c{c}_p{i}_den_cb"], out[f"c{c}_p{i}_den_cr"] = r["out_cb"], r["out_cr"]
                    for k in nu.DETECT_OUTPUTS:
                        out[f"c{c}_p{i}_s{sub}_{k}"] = r[k]
                seen.append((w, h, luma, cb, cr, ref))
                print("case", c, (w, h), name, "picture", [tuple(int(v) for v in ref[s]["picture"]) for s in (0, 1)], "flat", int(ref[1]["flat_noise"].sum()))
    cov = nu.coverage(seen)
    print("coverage", cov)
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    out["coverage_keys"] = np.array(nu.COVERAGE_KEYS, dtype="U40")
    save(nu.FIXTURE, out)
    print(f"wrote {nu.FIXTURE}: {os.path.getsize(nu.FIXTURE) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
