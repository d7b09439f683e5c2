"""Writes tests/golden/cdef128.npz from the reference's own CDEF strength search, strength pick and frame filter on grids with 128-wide
blocks (tests/golden/ref_cdef128_driver.c, linked by the recipe of oracle/ref_driver.py against the reference objects of the oracle build).
Run in the build container only, where the reference exists: the fixture is data.

    python tests/golden/make_golden_cdef128.py

Pictures and deblocked pictures are make_golden_cdef.py's constructions.  Cases (tests/cdef128_util.py: CASES, make_grid, make_skip), each
at 8 and at 10 bits and three base_qindex values with different dampings: A one BLOCK_128X128; B 328x200 with every wide type, full and
clipped, over small blocks; C a grid whose first cells contradict each other; D B's picture with nothing 128 wide; E 3 x 3 fbs of
128X128, whose copies leave the picture.
  case, case_name, case_picture        width, height, bit depth; the name; the case whose planes and skip map the case uses (D uses B's)
  qindex                               the three base_qindex values
  c{c}_src_{p}, c{c}_dbk_d{p}, c{c}_skip   as in cdef.npz (only where case_picture[c] == c)
  c{c}_sb_type                         [h / 4][w / 4] bytes: BlockSize per cell
  c{c}_mse, c{c}_counted               [3 qindex][2][nfb][64] what cdef_seg_search[16bit] left in mse_seg; [nfb] 1 for an fb that is searched
  c{c}_result, c{c}_fb_strength        [3] finish_cdef_search's result as 21 int32; [3][nfb] cdef_strength of each fb's first cell, -1 untouched
  c{c}_run_result, c{c}_run_fb_strength   the frame-filter runs: 0 the search's own result at qindex[0]; 1 eight constructed pairs with
                                       pri_damping != sec_damping on the fbs run 0 gave an index
  c{c}_out{r}_d{p}                     what av1_cdef_frame[16bit] left of plane p in run r, minus the deblocked plane
  coverage_keys                        cdef128_util.COVERAGE_KEYS, every one asserted here and by tests/test_cdef128_vs_ref.py
The restatement (tests/cdef128_util.py) is asserted equal to the reference on every case, table, pick and output plane."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import cdef128_util as c128  # noqa: E402
import cdef_util as cu  # noqa: E402
from make_golden_cdef import constructed_runs, make_pictures, save  # noqa: E402
from make_golden_lr import _ptrs, delta  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

OUT = os.path.join(HERE, "cdef128.npz")


def build_driver(out_dir):
    """ref_cdef128_driver.c by the recipe of oracle/ref_driver.py, with its signatures."""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_cdef128_driver.c"), out_dir)
    V = C.c_void_p
    L.drv_cdef128_open.argtypes = [C.c_int] * 3 + [V] * 4
    L.drv_cdef128_search.argtypes = [C.c_int, V]
    L.drv_cdef128_finish.argtypes = [C.c_int, V, V, V]
    L.drv_cdef128_frame.argtypes = [V, V, V]
    return L


class Reference:
    """one opened picture in the driver"""

    def __init__(self, L, w, h, bd, dbk, src, skip, sb_type):
        self.L, self.w, self.h, self.bd = L, w, h, bd
        self.keep = [np.ascontiguousarray(p) for s in (dbk, src) for p in s] + [np.ascontiguousarray(skip, np.uint8), np.ascontiguousarray(sb_type, np.uint8)]
        self.nfb = L.drv_cdef128_open(w, h, bd, _ptrs(self.keep[0:3]), _ptrs(self.keep[3:6]), self.keep[6].ctypes.data, self.keep[7].ctypes.data)
        assert self.nfb == cu.geometry(w, h)[0] * cu.geometry(w, h)[1]

    def close(self):
        self.L.drv_cdef128_close()

    def search(self, q):
        mse = np.zeros((2, self.nfb, 64), np.uint64)
        assert self.L.drv_cdef128_search(q, mse.ctypes.data) == 0
        return mse

    def finish(self, q, mse=None):
        res, fbs = np.zeros(21, np.int32), np.zeros(self.nfb, np.int8)
        m = None if mse is None else np.ascontiguousarray(mse, np.uint64)
        assert self.L.drv_cdef128_finish(q, None if m is None else m.ctypes.data, res.ctypes.data, fbs.ctypes.data) == 0
        return res.view(cu.RESULT_DTYPE)[0], fbs

    def frame(self, res, fbs):
        dt = np.uint16 if self.bd > 8 else np.uint8
        out = [np.zeros((self.h >> (p > 0), self.w >> (p > 0)), dt) for p in range(3)]
        r, f = np.ascontiguousarray(np.asarray(res).reshape(1).view(np.int32)), np.ascontiguousarray(fbs, np.int8)
        assert self.L.drv_cdef128_frame(r.ctypes.data, f.ctypes.data, _ptrs(out)) == 0
        return out


def check_case(R, F, qi):
    """the restatement against the opened reference for qindex qi -> (mse, counted, result, fb_strength) of the reference"""
    q = F["qindex"][qi]
    ref_mse = R.search(q)
    ref_res, ref_fbs = R.finish(q)
    mse, counted = c128.search(F["dbk"], F["src"], F["skip"], F["sb_type"], F["w"], F["h"], F["bd"], q)
    assert np.array_equal(mse, ref_mse), ("the restatement's tables differ from the reference's", F["name"], F["bd"], q)
    res, fbs = c128.pick(mse, counted, F["sb_type"], F["w"], F["h"], q, F["bd"])
    assert res == ref_res and np.array_equal(fbs, ref_fbs), ("the restatement's pick differs", F["name"], F["bd"], q, res, ref_res, fbs, ref_fbs)
    return ref_mse, counted, ref_res, ref_fbs


def check_frame(R, F, res, fbs):
    got = R.frame(res, fbs)
    mine = c128.frame(F["dbk"], F["skip"], F["w"], F["h"], F["bd"], res, fbs)
    for p in range(3):
        assert np.array_equal(got[p], mine[p]), ("the restatement's frame filter differs from the reference's", F["name"], F["bd"], p)
    return got


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    rng = np.random.default_rng(20261021)
    out = {"case": np.array([c[1:] for c in c128.CASES], np.int32), "case_name": np.array([c[0] for c in c128.CASES], dtype="U1"),
           "qindex": np.array(c128.QINDEX, np.int32)}
    pictures, share, loaded = {}, [], []
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for c, (name, w, h, bd) in enumerate(c128.CASES):
            key = ("B" if name == "D" else name, bd)
            if key not in pictures:
                dbk, src = make_pictures(rng, w, h, bd)
                pictures[key] = (c, dbk, src, c128.make_skip(rng, name, w, h))
                for p in range(3):
                    out[f"c{c}_src_{p}"], out[f"c{c}_dbk_d{p}"] = src[p], delta(dbk[p], src[p])
                out[f"c{c}_skip"] = pictures[key][3]
            at, dbk, src, skip = pictures[key]
            share.append(at)
            F = {"name": name, "w": w, "h": h, "bd": bd, "dbk": dbk, "src": src, "skip": skip, "sb_type": c128.make_grid(name, w, h), "qindex": list(c128.QINDEX)}
            F["nhfb"], F["nvfb"] = cu.geometry(w, h)
            R = Reference(L, w, h, bd, dbk, src, skip, F["sb_type"])
            per_q = [check_case(R, F, qi) for qi in range(len(c128.QINDEX))]
            F["mse"], F["counted"] = np.array([p[0] for p in per_q]), per_q[0][1]
            F["result"], F["fb_strength"] = np.array([p[2] for p in per_q]), np.array([p[3] for p in per_q], np.int8)
            on = (F["fb_strength"][0] >= 0).astype(np.uint8)
            runs = [(F["result"][0], F["fb_strength"][0]), constructed_runs(rng, on)[0]]
            for r, (res, fbs) in enumerate(runs):
                got = check_frame(R, F, res, fbs)
                for p in range(3):
                    out[f"c{c}_out{r}_d{p}"] = delta(got[p], dbk[p])
            R.close()
            if name == "D":      # the equality with the existing treatment
                m64, c64, _, _ = cu.search(dbk, src, skip, w, h, bd, c128.QINDEX[0])
                assert np.array_equal(m64, F["mse"][0]) and np.array_equal(c64, F["counted"])
            out[f"c{c}_sb_type"], out[f"c{c}_mse"], out[f"c{c}_counted"] = F["sb_type"], F["mse"], F["counted"]
            out[f"c{c}_result"] = F["result"].view(np.int32).reshape(len(c128.QINDEX), 21)
            out[f"c{c}_fb_strength"] = F["fb_strength"]
            out[f"c{c}_run_result"] = np.array([r[0] for r in runs]).view(np.int32).reshape(len(runs), 21)
            out[f"c{c}_run_fb_strength"] = np.array([r[1] for r in runs], np.int8)
            loaded.append(F)
            print("case", c, (name, w, h, bd), "counted", F["counted"].tolist(), "fb_strength", F["fb_strength"][0].tolist(),
                  "bits", [int(r["cdef_bits"]) for r in F["result"]], flush=True)
    out["case_picture"] = np.array(share, np.int32)
    cov = c128.coverage(loaded)
    print("coverage", cov)
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    out["coverage_keys"] = np.array(c128.COVERAGE_KEYS, dtype="U48")
    save(OUT, out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
