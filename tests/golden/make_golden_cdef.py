"""Writes tests/golden/cdef.npz from the reference's own CDEF strength search, strength pick and frame filter (tests/golden/ref_cdef_driver.c,
linked by the recipe of oracle/ref_driver.py against the reference objects of the oracle build, oracle/_ref/obj_all).  Run in the build
container only, where the reference exists: the fixture is data.

    python tests/golden/make_golden_cdef.py

Pictures are synthetic: the source is a patchwork of 32x32 zones of strong edges, one orientation per zone over all eight CDEF directions,
with flat patches at 0 and at the maximum; the deblocked picture is the source blurred, coarsely quantised and ringing a little.
Contents, per case c (`case` holds width, height, bit depth per row; 64x64, 200x136, 136x200 at 8 and at 10 bits):
  c{c}_src_{p}, c{c}_dbk_d{p}          the source planes; deblocked - source (cdef_util.load_case adds them up)
  c{c}_skip                            [h / 4][w / 4] bytes, non-zero = mbmi->skip: random cells; from the second picture on one fb entirely
                                       skipped and one with a single listed block; the 8-bit 136x200 picture has nothing skipped
  c{c}_qindex                          three base_qindex values with different dampings
  c{c}_mse, c{c}_counted               [3 qindex][2][nfb][64] what cdef_seg_search[16bit] left in mse_seg; [nfb] sb_all_skip is false
  c{c}_dir_fb, c{c}_dirs, c{c}_vars    one fb and its [8][8] directions and variances from the dispatched cdef_find_dir (-1 outside the picture)
  c{c}_result, c{c}_fb_strength        [3 qindex] finish_cdef_search's result as 21 int32 (cdef_util.RESULT_DTYPE); [3][nfb] picked index, -1 left out
  c{c}_run_result, c{c}_run_fb_strength   the frame-filter runs: 0 the search's own result at qindex[0]; 1 eight constructed pairs, one of
                                       them (0, 0) and selected by some fbs, with pri_damping != sec_damping; 2 luma (0, 0) with chroma non-zero
  c{c}_out{r}_d{p}                     what av1_cdef_frame[16bit] left of plane p in run r, minus the deblocked plane
Dist pairs: dist{bd}_dst, dist{bd}_src [n][64] uint16, dist{bd}_ref [n] uint64 from the dispatched dist_8x8_16bit: constant blocks, equal
blocks, extremes, textured blocks with small and large differences.
Constructed pick tables answered by the restatement alone (tests/cdef_util.py), marked `synthetic`: syn_mse [t][2][6][64], syn_counted,
syn_qindex, syn_result, syn_fb_strength for a 3 x 2 grid of fbs: exact ties between (j, k) pairs and, at qindex 0 where both lambda terms
truncate to 0, between values of i.
setup_rtcd_internal(ASM_AVX2) as the encoder: tests/cdef_util.py restates the C forms, so every equality with this fixture is also a check of
C against AVX2.  Coverage: coverage() below, asserted here and by tests/test_cdef_vs_ref.py::test_fixture_covers_the_ground."""
import ctypes as C
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import cdef_util as cu  # noqa: E402
from make_golden_lr import _ptrs, delta  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

OUT = os.path.join(HERE, "cdef.npz")
CASES = ((64, 64, 8), (200, 136, 8), (136, 200, 8), (64, 64, 10), (200, 136, 10), (136, 200, 10))
QINDEX = (20, 100, 255)
N_RUNS = 3


def build_driver(out_dir):
    """ref_cdef_driver.c by the recipe of oracle/ref_driver.py, with its signatures."""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_cdef_driver.c"), out_dir)
    V = C.c_void_p
    L.drv_cdef_open.argtypes = [C.c_int] * 3 + [V] * 3
    L.drv_cdef_search.argtypes = [C.c_int, V]
    L.drv_cdef_finish.argtypes = [C.c_int, V, V, V]
    L.drv_cdef_frame.argtypes = [V, V, V]
    L.drv_cdef_dirs.argtypes = [C.c_int, V, V]
    L.drv_cdef_dist.argtypes = [V, V, C.c_int, C.c_int, V]
    L.drv_cdef_time.restype = C.c_double
    L.drv_cdef_time.argtypes = [C.c_int, V]
    return L


class Reference:
    """one opened picture in the driver"""

    def __init__(self, L, w, h, bd, dbk, src, skip):
        self.L, self.w, self.h, self.bd = L, w, h, bd
        self.keep = [np.ascontiguousarray(p) for s in (dbk, src) for p in s] + [np.ascontiguousarray(skip, np.uint8)]
        self.nfb = L.drv_cdef_open(w, h, bd, _ptrs(self.keep[0:3]), _ptrs(self.keep[3:6]), self.keep[6].ctypes.data)
        assert self.nfb == cu.geometry(w, h)[0] * cu.geometry(w, h)[1]

    def close(self):
        self.L.drv_cdef_close()

    def search(self, q):
        mse = np.zeros((2, self.nfb, 64), np.uint64)
        assert self.L.drv_cdef_search(q, mse.ctypes.data) == 0
        return mse

    def finish(self, q, mse=None):
        res, fbs = np.zeros(21, np.int32), np.zeros(self.nfb, np.int8)
        m = None if mse is None else np.ascontiguousarray(mse, np.uint64)
        assert self.L.drv_cdef_finish(q, None if m is None else m.ctypes.data, res.ctypes.data, fbs.ctypes.data) == 0
        return res.view(cu.RESULT_DTYPE)[0], fbs

    def frame(self, res, fbs):
        dt = np.uint16 if self.bd > 8 else np.uint8
        out = [np.zeros((self.h >> (p > 0), self.w >> (p > 0)), dt) for p in range(3)]
        r, f = np.ascontiguousarray(np.asarray(res).reshape(1).view(np.int32)), np.ascontiguousarray(fbs, np.int8)
        assert self.L.drv_cdef_frame(r.ctypes.data, f.ctypes.data, _ptrs(out)) == 0
        return out

    def dirs(self, fb):
        d, v = np.full(64, -1, np.int32), np.full(64, -1, np.int32)
        self.L.drv_cdef_dirs(fb, d.ctypes.data, v.ctypes.data)
        return d, v

    def time(self, q):
        parts = np.zeros(3)
        return self.L.drv_cdef_time(q, parts.ctypes.data), parts


def make_pictures(rng, w, h, bd):
    """source and deblocked planes: low-entropy constructions so that the fixture compresses"""
    top, sh = (1 << bd) - 1, bd - 8
    dt = np.uint16 if bd > 8 else np.uint8
    src, dbk = [], []
    for p in range(3):
        pw, ph = w >> (p > 0), h >> (p > 0)
        zone = 32 >> (p > 0)
        y, x = np.mgrid[0:ph, 0:pw]
        z = (x // zone + 3 * (y // zone)) % 8
        ang = np.pi * (2 - z) / 8.0 + np.pi / 2          # the normal of an edge along CDEF direction z
        f = 128 + 80 * np.sign(np.sin((x * np.cos(ang) + y * np.sin(ang)) * (0.9 - 0.2 * p) + 0.3)) + 12 * np.sin(x * 1.7 + y * 1.1)
        zf = (x // zone + 2 * (y // zone)) % 7 == 3        # flat zones: var == 0
        f[zf] = 64 + 16 * p
        for k in range(4):                                 # saturated patches, black and white, with a line of the other extreme
            cx, cy, v = int(rng.integers(0, pw)), int(rng.integers(0, ph)), k % 2
            f[max(cy - 5, 0):cy + 5, max(cx - 8, 0):cx + 8] = 400 * v - 100
            f[max(cy - 5, 0):cy + 5, cx:cx + 1] = 300 - 400 * v
        s = np.clip(np.round(f / 4) * 4, 0, 255).astype(np.int64) << sh
        s[s >= (252 << sh)] = top
        pad = np.pad(s, 1, mode="edge")
        blur = (pad[1:-1, 1:-1] * 4 + pad[:-2, 1:-1] + pad[2:, 1:-1] + pad[1:-1, :-2] + pad[1:-1, 2:]) // 8
        q = 8 << sh
        d = np.clip((blur + (q >> 1)) // q * q + (((x * 3 + y * 5) % 7 == 0) * 6 - ((x * 5 + y * 3) % 11 == 0) * 5) * (1 << sh), 0, top)
        d[s == 0], d[s == top] = 0, top
        d[zf] = s[zf]
        src.append(s.astype(dt)), dbk.append(d.astype(dt))
    return dbk, src


def make_skip(rng, c, w, h):
    mr, mc = h >> 2, w >> 2
    nh, nv = cu.geometry(w, h)
    if CASES[c] == (136, 200, 8):
        return np.zeros((mr, mc), np.uint8)
    skip = (rng.random((mr, mc)) < 0.55).astype(np.uint8)
    skip[0:2, 0:2] = (1, 0), (1, 1)                     # a block with three skipped cells is still listed
    if nh * nv > 1:
        skip[0:16, 16:32] = 1                           # fb 1 entirely skipped
        r0, c0 = (nv - 1) * 16, 0                       # the first fb of the last row: one listed block
        skip[r0:r0 + 16, c0:c0 + 16] = 1
        skip[r0, c0 + 1] = 0
    return skip


def constructed_runs(rng, counted):
    n = len(counted)
    a = np.zeros((), cu.RESULT_DTYPE)
    a["cdef_bits"], a["nb_cdef_strengths"], a["pri_damping"], a["sec_damping"], a["sb_count"] = 3, 8, 5, 4, int(counted.sum())
    a["cdef_strengths"] = (63, 5, 16, 0, 2, 44, 33, 7)
    a["cdef_uv_strengths"] = (12, 3, 60, 0, 1, 19, 0, 40)
    fa = np.where(counted != 0, rng.integers(0, 8, n), -1).astype(np.int8)
    on = np.flatnonzero(counted)
    fa[on[0]] = 0
    if len(on) > 2:
        fa[on[1]], fa[on[2]] = 3, 6
    b = np.zeros((), cu.RESULT_DTYPE)
    b["cdef_bits"], b["nb_cdef_strengths"], b["pri_damping"], b["sec_damping"], b["sb_count"] = 1, 2, 4, 4, int(counted.sum())
    b["cdef_uv_strengths"][:2] = (5, 37)
    fb = np.where(counted != 0, rng.integers(0, 2, n), -1).astype(np.int8)
    return [(a, fa), (b, fb)]


def dist_pairs(rng, bd, n_random=1500):
    top = (1 << bd) - 1
    dst, src = [], []
    consts = (0, 1, top // 2, top - 1, top)
    for a in consts:
        for b in consts:
            dst.append(np.full(64, a)), src.append(np.full(64, b))
    chk = ((np.arange(64) // 8 + np.arange(64)) % 2) * top
    ramp = np.arange(64) * top // 63
    for a in (chk, top - chk, ramp, ramp[::-1]):
        for b in (chk, top - chk, ramp, np.full(64, 0), np.full(64, top)):
            dst.append(a), src.append(b)
    for i in range(n_random):
        base = int(rng.integers(0, top + 1))
        amp = (1, 4, 16, 64)[i % 4] << (bd - 8)
        s = np.clip(base + rng.integers(-amp, amp + 1, 64) // (1 + i % 3) * (1 + i % 3), 0, top)
        if i % 5 == 0:
            d = s.copy()                                           # equal blocks
        else:
            d = np.clip(s + rng.integers(-(1 + i % 7), 2 + i % 7, 64) * (1 << (bd - 8)) * (1 + 8 * (i % 11 == 0)), 0, top)
        dst.append(d), src.append(s)
    return np.array(dst, np.uint16), np.array(src, np.uint16)


def synthetic_tables(rng):
    """[(mse [2][6][64], counted [6], qindex)]"""
    counted = np.array([1, 1, 0, 1, 1, 1], np.uint8)
    out = []
    flat = np.full((2, 6, 64), 1000, np.uint64)
    out.append((flat, counted, 0))                                   # every (j, k) and every i ties: (0, 0), i = 0
    two = np.full((2, 6, 64), 500, np.uint64)
    two[0, :, 9] = two[0, :, 5] = 100
    two[1, :, 7] = two[1, :, 3] = 50
    out.append((two, counted, 0))                                    # four tied pairs: (5, 3)
    for k, q in enumerate((0, 0, 0, 60, 255)):
        m = rng.integers(0, 3 + 2 * k, (2, 6, 64)).astype(np.uint64) * np.uint64(10 if q else 1)
        out.append((m, counted, q))
    half = np.full((2, 6, 64), 900, np.uint64)                        # two groups of fbs, each with two tied best pairs
    half[0, :2, 20] = half[0, :2, 8] = 10
    half[0, 3:, 40] = half[0, 3:, 33] = 10
    half[1, :, 2] = half[1, :, 1] = 10
    out.append((half, counted, 0))
    out.append((half, np.zeros(6, np.uint8), 0))                      # nothing counted
    for (m, cnt, q) in out:
        m[:, cnt == 0, :] = 0
    return out


def coverage(st, flags):
    """what of the issue's list the recorded runs do not reach (names)"""
    return [k for k in cu.STAT_KEYS if not st[k]] + [k for k, v in flags.items() if not v]


def save(path, arrays):
    """an .npz with fixed entry dates, so that the same data gives the same file"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            bio = io.BytesIO()
            np.lib.format.write_array(bio, np.asanyarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, bio.getvalue())


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    rng = np.random.default_rng(20261019)
    out = {"case": np.array(CASES, np.int32)}
    st = cu.new_stats()
    flags = {"partly_skipped_block_listed": False, "fb_all_skipped": False, "fb_single_block": False, "nothing_skipped": False,
             "var_zero": False, "sample_zero": False, "sample_max": False, "lambda_changes_bits": False, "narrow_fb": False, "low_fb": False}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for c, (w, h, bd) in enumerate(CASES):
            dbk, src = make_pictures(rng, w, h, bd)
            skip = make_skip(rng, c, w, h)
            nh, nv = cu.geometry(w, h)
            R = Reference(L, w, h, bd, dbk, src, skip)
            listed, counted2 = cu.block_lists(skip, w, h)
            mses, results, fbss = [], [], []
            for qi, q in enumerate(QINDEX):
                ref_mse = R.search(q)
                ref_res, ref_fbs = R.finish(q)
                mse, counted, dirs, variances = cu.search(dbk, src, skip, w, h, bd, q, st)
                assert np.array_equal(mse, ref_mse), ("the restatement's tables differ from the reference's", c, q)
                assert np.array_equal(counted != 0, ref_fbs >= 0), (c, q)
                res, fbs = cu.pick(mse, counted, q, bd)
                assert res == ref_res and np.array_equal(fbs, ref_fbs), ("the restatement's pick differs", c, q, res, ref_res, fbs, ref_fbs)
                flags["lambda_changes_bits"] |= int(cu.pick(mse, counted, q, bd, lam=0.0)[0]["cdef_bits"]) != int(res["cdef_bits"])
                mses.append(ref_mse), results.append(ref_res), fbss.append(ref_fbs)
            dir_fb = R.nfb - 1 if R.nfb > 1 else 0          # the last fb: 8 wide and 8 high in the larger pictures
            rd, rv = R.dirs(dir_fb)
            r0, c0 = dir_fb // nh * 8, dir_fb % nh * 8
            md, mv = np.full((8, 8), -1, np.int32), np.full((8, 8), -1, np.int32)
            sub = dirs[r0:r0 + 8, c0:c0 + 8]
            md[:sub.shape[0], :sub.shape[1]], mv[:sub.shape[0], :sub.shape[1]] = sub, variances[r0:r0 + 8, c0:c0 + 8]
            assert np.array_equal(md.reshape(-1), rd) and np.array_equal(mv.reshape(-1), rv), ("directions differ", c)
            runs = [(results[0], fbss[0])] + constructed_runs(rng, counted)
            for r, (res, fbs) in enumerate(runs):
                got = R.frame(res, fbs)
                mine = cu.frame(dbk, skip, w, h, bd, res, fbs, st)
                for p in range(3):
                    assert np.array_equal(got[p], mine[p]), ("the restatement's frame filter differs from the reference's", c, r, p)
                    out[f"c{c}_out{r}_d{p}"] = delta(got[p], dbk[p])
            R.close()
            cells = listed.shape
            s4 = skip[:cells[0] * 2, :cells[1] * 2].reshape(cells[0], 2, cells[1], 2).sum((1, 3))
            flags["partly_skipped_block_listed"] |= bool(((s4 > 0) & (s4 < 4)).any())
            flags["fb_all_skipped"] |= bool((counted == 0).any())
            flags["fb_single_block"] |= any(listed[r * 8:(r + 1) * 8, k * 8:(k + 1) * 8].sum() == 1 for r in range(nv) for k in range(nh))
            flags["nothing_skipped"] |= not skip.any()
            flags["var_zero"] |= bool(((variances == 0) & listed).any())
            flags["sample_zero"] |= bool((dbk[0] == 0).any())
            flags["sample_max"] |= bool((dbk[0] == (1 << bd) - 1).any())
            flags["narrow_fb"] |= w % 64 == 8
            flags["low_fb"] |= h % 64 == 8
            for p in range(3):
                out[f"c{c}_src_{p}"], out[f"c{c}_dbk_d{p}"] = src[p], delta(dbk[p], src[p])
            out[f"c{c}_skip"], out[f"c{c}_qindex"] = skip, np.array(QINDEX, np.int32)
            out[f"c{c}_mse"], out[f"c{c}_counted"] = np.array(mses), counted
            out[f"c{c}_result"] = np.array(results).view(np.int32).reshape(len(QINDEX), 21)
            out[f"c{c}_fb_strength"] = np.array(fbss, np.int8)
            out[f"c{c}_dir_fb"], out[f"c{c}_dirs"], out[f"c{c}_vars"] = np.int32(dir_fb), rd, rv
            out[f"c{c}_run_result"] = np.array([r[0] for r in runs]).view(np.int32).reshape(N_RUNS, 21)
            out[f"c{c}_run_fb_strength"] = np.array([r[1] for r in runs], np.int8)
            print("case", c, (w, h, bd), "counted", counted.tolist(), "bits", [int(r["cdef_bits"]) for r in results])
        for bd in (8, 10):
            d, s = dist_pairs(rng, bd)
            ref = np.zeros(len(d), np.uint64)
            L.drv_cdef_dist(d.ctypes.data, s.ctypes.data, len(d), bd - 8, ref.ctypes.data)
            assert np.array_equal(ref, cu.dist_8x8(d, s, bd - 8)), ("dist_8x8 differs", bd)
            out[f"dist{bd}_dst"], out[f"dist{bd}_src"], out[f"dist{bd}_ref"] = d, s, ref
    unreached = coverage(st, flags)
    print("stats", st, "flags", flags, "unreached", unreached)
    assert not unreached, unreached
    out["coverage_keys"] = np.array(list(cu.STAT_KEYS) + list(flags), dtype="U32")
    syn = synthetic_tables(rng)
    picks = [cu.pick(m, cnt, q, 8) for (m, cnt, q) in syn]
    assert tuple(int(v) for v in picks[0][0]["cdef_strengths"][:1]) == (0,) and int(picks[0][0]["cdef_bits"]) == 0
    assert (int(picks[1][0]["cdef_strengths"][0]), int(picks[1][0]["cdef_uv_strengths"][0])) == (5, 3)
    out["syn_mse"], out["syn_counted"] = np.array([s[0] for s in syn]), np.array([s[1] for s in syn])
    out["syn_qindex"] = np.array([s[2] for s in syn], np.int32)
    out["syn_result"] = np.array([p[0] for p in picks]).view(np.int32).reshape(len(syn), 21)
    out["syn_fb_strength"] = np.array([p[1] for p in picks], np.int8)
    out["synthetic"] = np.array(["syn_mse", "syn_counted", "syn_qindex", "syn_result", "syn_fb_strength"], dtype="U16")
    save(OUT, out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
