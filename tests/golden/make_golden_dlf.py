"""Writes tests/golden/dlf.npz from the reference's own av1_loop_filter_frame, PictureSseCalculations and av1_pick_filter_level
(tests/golden/ref_dlf_driver.c linked against the reference objects of the oracle build, oracle/_ref/obj_all).  Run in the build container
only, where the reference exists: the fixture is data and is what the GPU box checks.

    python tests/golden/make_golden_dlf.py

Contents, per case c = 0 .. 5 (64x64, 136x72, 200x136 at 8 and 10 bits; `case` holds w, h, bit depth per row)
  c{c}_mi                        LF_MI_DTYPE grid, (superblock rows * 16) x (superblock columns * 16)
  c{c}_recon_{p}, c{c}_source_{p} the reconstructed and the source planes p = 0, 1, 2
  c{c}_run                       one row per frame filtering: the four levels, sharpness, plane_start, plane_end
  c{c}_out{r}_{p}                what av1_loop_filter_frame left of plane p in run r
  c{c}_table                     [5][64] av1_loop_filter_frame + PictureSseCalculations per level for the five searches of the pick
                                 (dlf_util.PICK_RUNS), each with the other levels as the reference's pick has them at that search
  c{c}_table_levels              [5][4] those other levels (the level array at the start of each search)
  c{c}_pick                      one row per pick: last_frame_filter_level[4], tx_mode == ONLY_4X4, the four levels av1_pick_filter_level left
  c{c}_pick{k}_trace             the four levels of every frame filtering pick k ran, in order (noted inside av1_loop_filter_frame)
  c{c}_pick{k}_mask              the levels each of its five walks tried, as bit masks (split from the trace by the restatement, whose
                                 trace is checked to be the reference's, entry by entry)
  walk_table, walk_arg, walk_out further tables: [n][64], (start level, only 4x4), (level, visited mask).  The first rows are the
                                 reference's tables of small extra pictures with the reference's own pick results; the rows with
                                 walk_synthetic set are constructed tables (ties, clamps) answered by the restatement alone
The leaf filters the reference dispatches are its SSE2 forms (EbDeblockingFilter.h:145-243); tests/dlf_util.py restates the C forms, so
every equality with this fixture is also a check of C against SSE2.
Coverage: coverage() below, asserted again by tests/test_dlf_vs_ref.py::test_fixture_covers_the_ground."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import dlf_util as du  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

OUT = os.path.join(HERE, "dlf.npz")
SIZES = ((64, 64), (136, 72), (200, 136))
RUNS = ((20, 33, 12, 50, 0, 0, 3), (0, 9, 0, 3, 0, 0, 3), (40, 25, 30, 63, 3, 0, 3), (12, 12, 7, 9, 0, 1, 3), (0, 0, 5, 5, 0, 0, 3), (7, 0, 63, 0, 5, 0, 2))
PICKS = ((0, 0, 0, 0, 0), (10, 10, 20, 5, 0), (63, 40, 2, 60, 1), (30, 17, 63, 16, 0))
N_EXTRA = 10


def build_driver(out_dir):
    """ref_dlf_driver.c by the recipe of oracle/ref_driver.py, with its signature."""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_dlf_driver.c"), out_dir)
    L.drv_dlf.restype = C.c_int
    L.drv_dlf.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return L


def _call(L, op, bd, mi, recon, source, levels, sharpness, ps, pe, only_4x4=0, trace_cap=0):
    h, w = recon[0].shape
    mi = np.ascontiguousarray(mi)
    rec = [np.ascontiguousarray(p.copy()) for p in recon]
    src = [np.ascontiguousarray(p) for p in source] if source is not None else [None] * 3
    lv = np.array(levels, np.int32)
    sse, n = np.zeros(1, np.uint64), np.zeros(1, np.int32)
    trace = np.zeros((max(trace_cap, 1), 4), np.int32)
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    rc = L.drv_dlf(op, w, h, bd, mi.ctypes.data, mi.shape[0], mi.shape[1], ptr(rec[0]), ptr(rec[1]), ptr(rec[2]), ptr(src[0]), ptr(src[1]),
                   ptr(src[2]), lv.ctypes.data, sharpness, ps, pe, only_4x4, sse.ctypes.data, trace.ctypes.data, trace_cap, n.ctypes.data)
    assert rc == 0, rc
    return rec, [int(v) for v in lv], int(sse[0]), trace[:int(n[0])]


def reference_filter(L, bd, mi, recon, levels, sharpness, ps, pe):
    return _call(L, 0, bd, mi, recon, None, levels, sharpness, ps, pe)[0]


def reference_table(L, bd, mi, recon, source, plane, direction, levels, sharpness=0):
    return np.array([_call(L, 2, bd, mi, recon, source, du.try_levels(levels, plane, direction, lvl), sharpness, plane, plane + 1)[2]
                     for lvl in range(64)], np.uint64)


def reference_pick(L, bd, mi, recon, source, last_levels, only_4x4):
    rec, lv, _, trace = _call(L, 1, bd, mi, recon, source, last_levels, 0, 0, 3, only_4x4, trace_cap=512)
    assert all(np.array_equal(a, b) for a, b in zip(rec, recon)), "av1_pick_filter_level left the reconstruction changed"
    return lv, trace


def reference_pick_tables(L, bd, mi, recon, source, last_levels, only_4x4):
    """the five full tables at the levels the reference's own pick has when it starts each search, and those levels"""
    levels = [int(v) for v in last_levels]
    tables, at = [], []
    for (plane, direction, start, store) in du.PICK_RUNS:
        at.append(list(levels))
        t = reference_table(L, bd, mi, recon, source, plane, direction, levels)
        tables.append(t)
        best, _, _ = du.level_walk(t, last_levels[start], only_4x4)
        for k in store:
            levels[k] = best
    return np.array(tables), np.array(at, np.int32), levels


def make_case(rng, w, h, bd):
    mi = du.random_mi_grid(rng, w, h)
    recon, source = du.random_picture(rng, w, h, bd, mi)
    return mi, recon, source


def synthetic_walks(rng):
    """constructed tables: all equal (every comparison ties), strictly falling and rising (the walk runs into 63 and 0), a shallow bowl
    whose differences sit inside the bias, and noise on a large base"""
    rows = []
    lv = np.arange(64, dtype=np.int64)
    for base in (1 << 20, 1 << 34):
        shapes = [np.full(64, base), base - lv * 1000, base + lv * 1000, base + (lv - 21) ** 2 * (base >> 16), base + (lv - 40) ** 2,
                  base + rng.integers(-(base >> 12), base >> 12, 64), base - lv * (base >> 13), base + np.abs(lv - 9) * (base >> 11)]
        for t in shapes:
            for start in (0, 5, 15, 16, 33, 63):
                for only in (0, 1):
                    rows.append((np.asarray(t, np.uint64), start, only))
    return rows


def coverage(cases, walk_stats):
    """None when the fixture covers what the issue lists, else what is missing (from the restatement's statistics)"""
    st = du.new_stats()
    sharp = set()
    lvl0_one_dir = chroma0 = False
    for (w, h, bd, mi, recon, source) in cases:
        for (l0, l1, lu, lv, sharpness, ps, pe) in RUNS:
            du.loop_filter_frame([p.copy() for p in recon], mi, (l0, l1, lu, lv), sharpness, ps, pe, bd, st=st)
            sharp.add(sharpness > 0)
            lvl0_one_dir |= (l0 == 0) != (l1 == 0)
            chroma0 |= (lu == 0 or lv == 0) and (l0 or l1)
    want = {(0, d, n) for d in (0, 1) for n in (4, 8, 14)} | {(p, d, n) for p in (1, 2) for d in (0, 1) for n in (4, 6)}
    for k in ("len", "mask_fail", "hev", "no_hev"):
        if st[k] != want:
            return (k, want - st[k])
    wide = {k for k in want if k[2] > 4}
    if st["flat"] != wide or st["no_flat"] != wide:
        return ("flat", wide - st["flat"], wide - st["no_flat"])
    w14 = {k for k in want if k[2] == 14}
    if st["flat2"] != w14 or st["no_flat2"] != w14:
        return ("flat2", w14 - st["flat2"], w14 - st["no_flat2"])
    for k in ("clamp_lo", "clamp_hi", "skip_both_pu", "skip_both_inner", "skip_one"):
        if not st[k]:
            return (k,)
    every = {(p, d) for p in range(3) for d in (0, 1)}
    if st["sb_edge"] != every or st["partial_sb_edge"] != every:
        return ("sb edges", every - st["sb_edge"], every - st["partial_sb_edge"])
    tx = set(int(v) for (_, _, _, mi, _, _) in cases for v in np.unique(mi["tx_size"]))
    sb = set(int(v) for (_, _, _, mi, _, _) in cases for v in np.unique(mi["sb_type"]))
    if not {du.TX_OF[k] for k in ((4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16))} <= tx:
        return ("rectangular transforms", tx)
    if not {du.BLOCK_OF[k] for k in ((4, 4), (4, 8), (8, 4), (4, 16), (16, 4), (64, 64), (64, 32), (64, 16))} <= sb:
        return ("block sizes", sb)
    if not (sharp == {False, True} and lvl0_one_dir and chroma0):
        return ("levels", sharp, lvl0_one_dir, chroma0)
    for only in (0, 1):
        missing = [k for k, v in walk_stats[only].items() if not v]
        if missing:
            return ("walk", only, missing)
    return None


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for seed in range(20261018, 20261018 + 12):
            rng = np.random.default_rng(seed)
            cases = [(w, h, bd, *make_case(rng, w, h, bd)) for bd in (8, 10) for (w, h) in SIZES]
            extra = [(64, 64, (8, 10)[i % 2], *make_case(rng, 64, 64, (8, 10)[i % 2])) for i in range(N_EXTRA)]
            # the walks: the restatement's picks over everything, for the statistics only
            ws = {0: du.new_walk_stats(), 1: du.new_walk_stats()}
            jobs = [(c, p) for c in cases for p in PICKS] + [(c, PICKS[1 + i % 3]) for i, c in enumerate(extra)]
            for (w, h, bd, mi, recon, source), p in jobs:
                du.pick_filter_level(recon, source, mi, p[:4], 0, p[4], bd, st=ws[p[4]])
            syn = synthetic_walks(rng)
            for (t, start, only) in syn:
                du.level_walk(t, start, only, ws[only])
            missing = coverage(cases, ws)
            if missing is None:
                break
            print("seed", seed, "misses", missing)
        else:
            raise SystemExit("no seed met the coverage conditions")
        out = {"case": np.array([(w, h, bd) for (w, h, bd, *_) in cases], np.int32), "seed": np.array([seed])}
        for c, (w, h, bd, mi, recon, source) in enumerate(cases):
            out[f"c{c}_mi"] = mi
            out[f"c{c}_run"] = np.array(RUNS, np.int32)
            for p in range(3):
                out[f"c{c}_recon_{p}"], out[f"c{c}_source_{p}"] = recon[p], source[p]
            for r, (l0, l1, lu, lv, sharpness, ps, pe) in enumerate(RUNS):
                got = reference_filter(L, bd, mi, recon, (l0, l1, lu, lv), sharpness, ps, pe)
                for p in range(3):
                    out[f"c{c}_out{r}_{p}"] = got[p]
            out[f"c{c}_table"], out[f"c{c}_table_levels"], _ = reference_pick_tables(L, bd, mi, recon, source, PICKS[1][:4], PICKS[1][4])
            rows = []
            for k, p in enumerate(PICKS):
                lv, trace = reference_pick(L, bd, mi, recon, source, p[:4], p[4])
                o_lv, o_masks, o_trace = du.pick_filter_level(recon, source, mi, p[:4], 0, p[4], bd)
                assert np.array_equal(np.array(o_trace), trace), ("the restatement's pick ran other filterings than the reference's", c, k)
                assert o_lv == lv, (c, k, o_lv, lv)
                rows.append((*p, *lv))
                out[f"c{c}_pick{k}_trace"] = trace
                out[f"c{c}_pick{k}_mask"] = np.array(o_masks, np.uint64)
            out[f"c{c}_pick"] = np.array(rows, np.int32)
            print("case", c, (w, h, bd), "picks", [r[5:] for r in rows])
        wt, wa, wo, wsyn = [], [], [], []
        for i, (w, h, bd, mi, recon, source) in enumerate(extra):
            p = PICKS[1 + i % 3]
            tables, at, _ = reference_pick_tables(L, bd, mi, recon, source, p[:4], p[4])
            lv, trace = reference_pick(L, bd, mi, recon, source, p[:4], p[4])
            o_lv, o_masks, o_trace = du.pick_filter_level(None, None, None, p[:4], 0, p[4], bd, tables=tables)
            assert o_lv == lv and np.array_equal(np.array(o_trace), trace), ("walk over the reference's tables differs from its pick", i)
            for j, (plane, direction, start, store) in enumerate(du.PICK_RUNS):
                # the walk's own result: the pick above is the reference's, filtering by filtering, so each of its five walks ended here
                wt.append(tables[j]), wa.append((p[start], p[4])), wo.append((du.level_walk(tables[j], p[start], p[4])[0], o_masks[j])), wsyn.append(0)
        for (t, start, only) in syn:
            best, mask, _ = du.level_walk(t, start, only)
            wt.append(t), wa.append((start, only)), wo.append((best, mask)), wsyn.append(1)
        out["walk_table"], out["walk_arg"] = np.array(wt, np.uint64), np.array(wa, np.int32)
        out["walk_out"], out["walk_synthetic"] = np.array(wo, np.uint64), np.array(wsyn, np.uint8)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: seed {seed}, {len(cases)} cases, {len(wt)} walk tables, {os.path.getsize(OUT) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
