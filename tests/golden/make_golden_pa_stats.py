"""Writes tests/golden/pa_stats.npz from the reference's own GatheringPictureStatistics (tests/golden/ref_pa_stats_driver.c, linked by the
recipe of oracle/ref_driver.py against the reference objects of the oracle build, oracle/_ref/obj_all).  Run in the build container only,
where the reference exists: the fixture is data.

    python tests/golden/make_golden_pa_stats.py

Cases (tests/pa_stats_util.py CASES): 64x64 (one complete SB), 136x72 and 72x136 (a right column 8 wide, a bottom row 8 high, regions of
8 + 2 and 4 + 2 samples on the 1/16 plane, odd chroma region widths), 200x136, 320x192 (5 x 3 complete SBs, the homogeneity flags).
Pictures are constructed and low in entropy, see make_pictures.  Contents:
  case [5][2]                    width, height
  c{c}_n                         pictures of case c
  c{c}_p{i}_luma / _cb / _cr     the unpadded planes of picture i
  c{c}_p{i}_s{sub}_{output}      what the reference left, sub = 0 BLOCK_MEAN_PREC_FULL, 1 BLOCK_MEAN_PREC_SUB, output one of pa_stats_util.OUTPUTS
                                 (picture[3], the number of complete SBs, is counted by the driver from the reference's is_complete_sb)
  coverage_keys                  pa_stats_util.COVERAGE_KEYS, all reached: asserted here and by tests/test_pa_stats_vs_ref.py
asm_type is ASM_AVX2 as the encoder; the restatement (tests/pa_stats_util.py) is asserted equal to the reference on every output while
generating."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import pa_stats_util as pu  # noqa: E402
from make_golden_cdef import save  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


def build_driver(out_dir):
    """ref_pa_stats_driver.c by the recipe of oracle/ref_driver.py, with its signatures"""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_pa_stats_driver.c"), out_dir)
    V = C.c_void_p
    L.drv_pa_stats_open.argtypes = [C.c_int, C.c_int, V, V, V]
    L.drv_pa_stats_run.argtypes = [C.c_int] + [V] * 10
    L.drv_pa_stats_time.restype = C.c_double
    L.drv_pa_stats_time.argtypes = [C.c_int, C.c_int]
    return L


def reference_stats(L, luma, cb, cr):
    """{sub: outputs} of one picture from the driver"""
    h, w = luma.shape
    keep = [np.ascontiguousarray(p, np.uint8) for p in (luma, cb, cr)]
    n_sb = L.drv_pa_stats_open(w, h, *[p.ctypes.data for p in keep])
    assert n_sb == pu.sb_grid(w, h)[0] * pu.sb_grid(w, h)[1]
    outs = {}
    for sub in (0, 1):
        o = {"y_mean": np.zeros((n_sb, 85), np.uint8), "variance": np.zeros((n_sb, 85), np.uint16), "cb_mean": np.zeros((n_sb, 21), np.uint8),
             "cr_mean": np.zeros((n_sb, 21), np.uint8), "var_of_var": np.zeros((n_sb, 4), np.uint64), "homogeneous": np.zeros(n_sb, np.uint8),
             "picture": np.zeros(4, np.uint32), "histogram": np.zeros((4, 4, 3, 256), np.uint32), "region_intensity": np.zeros((4, 4, 3), np.uint32),
             "average_intensity": np.zeros(3, np.uint32)}
        assert L.drv_pa_stats_run(sub, *[o[k].ctypes.data for k in pu.OUTPUTS]) == 0
        outs[sub] = o
    L.drv_pa_stats_close()
    return outs


def _chroma(luma):
    return np.ascontiguousarray(luma[::2, ::2]), np.ascontiguousarray(255 - luma[1::2, 1::2])


def make_pictures(rng, w, h):
    """[(luma, cb, cr)]: noise at two amplitudes, flat 0, flat 255, an 8-pixel checkerboard of 0 and 255, a horizontal and a vertical ramp, a
    picture whose odd rows differ from its even rows; at 320x192 two more, built of SBs of quiet noise (64x64 variance below 5) and SBs whose
    8x8 variances differ widely: 13 and 10 of the 15 SBs quiet, for both values of both picture flags"""
    y, x = np.mgrid[0:h, 0:w]
    quiet = lambda: (128 + rng.integers(-1, 2, (h, w))).astype(np.uint8)  # noqa: E731
    pics = [quiet(), np.clip(120 + rng.integers(-5, 6, (h, w)) * 8, 0, 255).astype(np.uint8), np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8),
            ((((x >> 3) + (y >> 3)) & 1) * 255).astype(np.uint8), (x * 255 // (w - 1)).astype(np.uint8), (y * 255 // (h - 1)).astype(np.uint8),
            np.where(y & 1, 200 - (x & 31), 40 + (x & 15) * 3).astype(np.uint8)]
    if (w, h) == (320, 192):
        for n_quiet in (13, 10):
            p = quiet()
            for sb in range(n_quiet, 15):
                sy, sx = divmod(sb, 5)
                blk = p[sy * 64:(sy + 1) * 64, sx * 64:(sx + 1) * 64]
                if sb % 2:     # every other 8x8 block of strong noise: the 8x8 variances are far apart, the SB is not homogeneous
                    strong = np.clip(128 + rng.integers(-3, 4, (64, 64)) * 30, 0, 255).astype(np.uint8)
                    on = (((x[:64, :64] >> 3) + (y[:64, :64] >> 3)) & 1) == 1
                    blk[on] = strong[on]
                else:          # even noise: every 8x8 variance alike, the SB stays homogeneous
                    blk[:] = np.clip(128 + rng.integers(-2, 3, (64, 64)) * 10, 0, 255).astype(np.uint8)
            pics.append(p)
    return [(p, *_chroma(p)) for p in pics]


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    rng = np.random.default_rng(20261019)
    out = {"case": np.array(pu.CASES, np.int32)}
    seen = []
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for c, (w, h) in enumerate(pu.CASES):
            pics = make_pictures(rng, w, h)
            out[f"c{c}_n"] = np.int32(len(pics))
            for i, (luma, cb, cr) in enumerate(pics):
                ref = reference_stats(L, luma, cb, cr)
                for sub in (0, 1):
                    mine = pu.all_stats(luma, cb, cr, sub)
                    for k in pu.OUTPUTS:
                        assert np.array_equal(mine[k], ref[sub][k]), ("the restatement differs from the reference", (w, h), i, sub, k, mine[k], ref[sub][k])
                        out[f"c{c}_p{i}_s{sub}_{k}"] = ref[sub][k]
                out[f"c{c}_p{i}_luma"], out[f"c{c}_p{i}_cb"], out[f"c{c}_p{i}_cr"] = luma, cb, cr
                seen.append((w, h, luma, cb, cr, ref))
            print("case", c, (w, h), len(pics), "pictures; flags", [tuple(int(v) for v in s[5][1]["picture"]) for s in seen[-len(pics):]])
    cov = pu.coverage(seen)
    print("coverage", cov)
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    out["coverage_keys"] = np.array(pu.COVERAGE_KEYS, dtype="U32")
    save(pu.FIXTURE, out)
    print(f"wrote {pu.FIXTURE}: {os.path.getsize(pu.FIXTURE) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
