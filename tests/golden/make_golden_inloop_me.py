"""Writes tests/golden/inloop_me.npz from the reference's own in_loop_motion_estimation_sblock (tests/golden/ref_inloop_me_driver.c, linked by
the recipe of oracle/ref_driver.py against the reference objects of the oracle build, oracle/_ref/obj_all).  Run in the build container
only, where the reference exists: the fixture is data.

    python tests/golden/make_golden_inloop_me.py

Cases (tests/me_inloop_util.py make_cases), every one called with use_subpel_flag = 0 and with 1:
  random     136x72 (two full SB columns and one 8 wide, a full SB row and one 8 high), random source and references, area 64x64, both
             lists, centres that take every clip arm: left and top beyond -63, right and bottom, MAX(1, ..) with an area 1 wide and one
             1 high, widths that are no multiple of 4 (asserted below)
  small_odd  one SB, area 21x13        largest  one SB, area 127x127
  flat       flat source against flat references: every SAD ties, the first raster position wins
  extreme    source 0 against reference 255 on a full SB: the 20-bit SAD
  shifted    references equal to the source shifted by (+1.5, -0.25) and (-2.5, +3.25) samples
Contents: names; per case c: c{c}_src, c{c}_ref{l} (unpadded: the tests pad by edge replication, me_inloop_util.pad_plane), c{c}_lists,
c{c}_centers [lists][n_sb][2], c{c}_area [2], c{c}_desc [lists][n_sb][8] (the search areas; the offsets are those of the tests' planes),
c{c}_best_sad / c{c}_best_mv [lists][n_sb][849] (p_sb_best_sad / p_sb_best_mv), c{c}_inloop_mv [lists][n_sb][849][2] with use_subpel_flag = 0,
c{c}_sub_best_sad / _sub_best_mv / _sub_inloop_mv the same with 1, c{c}_sub_stale [lists][n_sb][849] bool, sub_stale_blocks their count;
ref_seconds_1080p / ref_seconds_1080p_subpel: the reference's time on one host thread for one 1080p picture, 510 SBs, one list, area
64x64, without and with the refinement.
Stale memory: every call is made twice, with p_sb_best_sad, p_sb_best_mv, inloop_me_mv, the three interpolated buffers of both lists and
avctemp_buffer pre-filled with 0x00 and then with 0xFF.  A block whose result differs between the two runs is one the reference computes
from bytes it never wrote: listed under c{c}_sub_stale, left out of every comparison, at most 1 % of the blocks of a case (asserted: a
condition on the inputs).  The restatement (tests/me_inloop_util.py) is asserted equal to everything else stored, and the generator asserts
that each of the four quarter-pel methods and each of the eight directions is taken by at least one block of the fixture."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import me_inloop_util as iu  # noqa: E402
from make_golden_cdef import save  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


REF_BORDER = 80   # the reference needs 65 or more (see the driver); the samples it reads are those of the tests' 64-sample border


def build_driver(out_dir):
    """ref_inloop_me_driver.c by the recipe of oracle/ref_driver.py, with its signatures"""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_inloop_me_driver.c"), out_dir)
    V = C.c_void_p
    L.drv_inloop_open.argtypes = [C.c_int, C.c_int, C.c_int, V, V, V]
    L.drv_inloop_run.argtypes = [C.c_int, C.c_int, V, C.c_int, C.c_int, C.c_int, C.c_int, V, V, V, V]
    L.drv_inloop_time.restype = C.c_double
    L.drv_inloop_time.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    return L


def reference_case(L, src, refs, ctr, area_w, area_h, use_subpel=0):
    """{origin [lists][n_sb][2], best_sad, best_mv [lists][n_sb][849], inloop_mv [lists][n_sb][849][2], stale [lists][n_sb][849] bool} from the
    driver.  Every SB is run with both pre-fills; a block whose result differs between them is one the reference computes from bytes it never
    wrote (`stale`), and is at most 1 % of the blocks of the case: asserted"""
    h, w = src.shape
    n_lists = len(refs)
    keep = [np.ascontiguousarray(src)] + [np.ascontiguousarray(iu.pad_plane(r, REF_BORDER)) for r in refs]
    n_sb = L.drv_inloop_open(w, h, REF_BORDER, keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data if n_lists == 2 else None)
    sbs = iu.sb_origins(w, h)
    assert n_sb == len(sbs)
    out = {"origin": np.zeros((n_lists, n_sb, 2), np.int16), "best_sad": np.zeros((n_lists, n_sb, iu.N_BLOCKS), np.uint32),
           "best_mv": np.zeros((n_lists, n_sb, iu.N_BLOCKS), np.uint32), "inloop_mv": np.zeros((n_lists, n_sb, iu.N_BLOCKS, 2), np.int16),
           "stale": np.zeros((n_lists, n_sb, iu.N_BLOCKS), bool)}
    for i, (sx, sy) in enumerate(sbs):
        c4 = np.zeros(4, np.int16)
        for l in range(n_lists):
            c4[2 * l:2 * l + 2] = ctr[l][i]
        runs = []
        for prefill in (0x00, 0xFF):
            o, s, m, p = np.zeros((2, 2), np.int16), np.zeros((2, iu.N_BLOCKS), np.uint32), np.zeros((2, iu.N_BLOCKS), np.uint32), \
                np.zeros((2, iu.N_BLOCKS, 2), np.int16)
            assert L.drv_inloop_run(int(sx), int(sy), c4.ctypes.data, area_w, area_h, use_subpel, prefill, o.ctypes.data, s.ctypes.data, m.ctypes.data,
                                    p.ctypes.data) == 0
            runs.append((o, s, m, p))
        assert np.array_equal(runs[0][0][:n_lists], runs[1][0][:n_lists])
        for l in range(n_lists):
            out["origin"][l, i], out["best_sad"][l, i], out["best_mv"][l, i], out["inloop_mv"][l, i] = (v[l] for v in runs[0])
            out["stale"][l, i] = (runs[0][1][l] != runs[1][1][l]) | (runs[0][2][l] != runs[1][2][l])
    assert out["stale"].sum() * 100 <= out["stale"].size, ("more than 1 % of the blocks depend on bytes the reference never wrote: change the case", int(out["stale"].sum()))
    return out


def clip_arms(ctr, sbs, w, h, area_w, area_h, desc):
    """which arms of :6389-6446 the case takes"""
    arms = set()
    for l in range(len(ctr)):
        for i, (sx, sy) in enumerate(sbs):
            for axis, (c, a, o, pic) in enumerate(((ctr[l][i][0], area_w, sx, w), (ctr[l][i][1], area_h, sy, h))):
                first = int(c) - (min(a, 127) >> 1)
                name = "xy"[axis]
                if o + first < -63:
                    arms.add(name + "_low")
                if o + first > pic - 1:
                    arms.add(name + "_high_origin")
                size = int(desc[l][i][4 + axis])
                if size < min(a, 127):
                    arms.add(name + "_high_size")
                if size == 1:
                    arms.add(name + "_one")
                if size % 4:
                    arms.add(name + "_not_multiple_of_4")
    return arms


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    cases = iu.make_cases()
    out = {"names": np.array([c[0] for c in cases], dtype="U16")}
    trace, stale_total = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for c, (name, src, refs, ctr, aw, ah) in enumerate(cases):
            ref = reference_case(L, src, refs, ctr, aw, ah)
            mine = iu.restate_case(src, refs, ctr, aw, ah)
            assert np.array_equal(mine["desc"][:, :, 2:4], ref["origin"]), ("the restatement's search-area origins differ", name)
            for k in ("best_sad", "best_mv", "inloop_mv"):
                assert np.array_equal(mine[k], ref[k]), ("the restatement differs from the reference", name, k, np.argwhere(mine[k] != ref[k])[:8])
            if name == "random":
                arms = clip_arms(ctr, iu.sb_origins(136, 72), 136, 72, aw, ah, mine["desc"])
                want = {a + b for a in "xy" for b in ("_low", "_high_origin", "_high_size", "_one")} | {"x_not_multiple_of_4"}
                assert want <= arms, sorted(want - arms)
            if name == "flat":   # every SAD ties: the first raster position wins
                assert all(np.array_equal(ref["best_mv"][l, i], np.full(iu.N_BLOCKS, ref["best_mv"][l, i, 0])) for l in range(2) for i in range(6))
            if name == "extreme":
                assert ref["best_sad"][0, 0, 340] == 64 * 64 * 255
            out[f"c{c}_src"], out[f"c{c}_lists"], out[f"c{c}_centers"], out[f"c{c}_area"] = src, np.int32(len(refs)), ctr, np.array([aw, ah], np.int32)
            for l, r in enumerate(refs):
                out[f"c{c}_ref{l}"] = r
            sub_ref = reference_case(L, src, refs, ctr, aw, ah, use_subpel=1)
            sub_mine = iu.restate_case(src, refs, ctr, aw, ah, use_subpel=True, trace=trace)
            keep = ~sub_ref["stale"]
            stale_total += int(sub_ref["stale"].sum())
            assert not ref["stale"].any()
            for k in ("best_sad", "best_mv"):
                assert np.array_equal(sub_mine[k][keep], sub_ref[k][keep]), ("the sub-pel restatement differs from the reference", name, k)
            assert np.array_equal(sub_mine["inloop_mv"][keep[:, :, iu.PACK_SOURCE]], sub_ref["inloop_mv"][keep[:, :, iu.PACK_SOURCE]]), (name, "inloop_mv")
            for k in ("best_sad", "best_mv", "inloop_mv"):
                out[f"c{c}_sub_{k}"] = sub_ref[k]
            out[f"c{c}_sub_stale"] = sub_ref["stale"]
            out[f"c{c}_desc"] = mine["desc"]
            for k in ("best_sad", "best_mv", "inloop_mv"):
                out[f"c{c}_{k}"] = ref[k]
            print("case", c, name, src.shape, "lists", len(refs), "areas", sorted({(int(d[4]), int(d[5])) for d in mine["desc"].reshape(-1, 8)}))
        # every quarter-pel method (the half-pel phase of the vector) and every psub_pel_direction is taken by some block of the fixture
        assert {m for m, _ in trace} == {0, 1, 2, 3} and {d for _, d in trace} == set(range(8)), sorted(set(trace))
        out["sub_stale_blocks"] = np.int32(stale_total)
        print("blocks whose sub-pel result depends on bytes the reference never wrote:", stale_total)
        # the CPU yardstick: one 1080p picture, 510 SBs, one list, 64x64, full-pel only
        rng = np.random.default_rng(7)
        big = rng.integers(0, 256, (1080, 1920), dtype=np.uint8)
        ref_big = np.ascontiguousarray(iu.pad_plane(np.roll(big, (3, -5), (0, 1)), REF_BORDER))
        assert L.drv_inloop_open(1920, 1080, REF_BORDER, big.ctypes.data, ref_big.ctypes.data, None) == 510
        out["ref_seconds_1080p"] = np.float64(min(L.drv_inloop_time(64, 64, 0, 1) for _ in range(2)))
        out["ref_seconds_1080p_subpel"] = np.float64(min(L.drv_inloop_time(64, 64, 1, 1) for _ in range(2)))
        print("the same with use_subpel_flag = 1:", float(out["ref_seconds_1080p_subpel"]), "s")
        print("reference, one host thread, 1080p, one list, 64x64, full-pel:", float(out["ref_seconds_1080p"]), "s")
    save(iu.FIXTURE, out)
    print(f"wrote {iu.FIXTURE}: {os.path.getsize(iu.FIXTURE) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
