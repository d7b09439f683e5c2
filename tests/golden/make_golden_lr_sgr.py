"""Writes tests/golden/lr_sgr.npz from the reference's own self-guided restoration search and frame filter (tests/golden/ref_lr_sgr_driver.c:
tests/golden/ref_lr_driver.c, i.e. the reference's EbRestorationPick.c included where it lies, plus calls; linked by the recipe of
oracle/ref_driver.py against oracle/_ref/obj_all without EbRestorationPick.o).  Run in the build container only, where the reference
exists: the fixture is data.

    python tests/golden/make_golden_lr_sgr.py

Pictures: cases 0-2 and 4-6 of tests/golden/lr.npz (64x64, 200x136, 136x200 at 8 and 10 bits), read through lr_util.load_case and not stored
again (`lr_case` holds their indices, -1 for a picture of this file), plus a 64x64 picture at 8 and at 10 bits whose CDEF'd Cb plane is
constant (ill-posed projection, default xq; 514 at 10 bits, a value whose rounded box sums give a * n < b * b) and whose CDEF'd Cr plane
equals the source (error 0 for every set: all sets tie and the first wins); its planes are x{c}_src_{p}, x{c}_dbk_d{p}, x{c}_cdef_d{p}.
Per case c
  c{c}_detail        [units][16] records (lr_sgr_util.DETAIL_DTYPE): the five sums, exq, start xqd, final xqd, err, n_trials
  c{c}_trace_xq, c{c}_trace_err   the trials of all walks in order, (unit, ep) after (unit, ep), split by min(n_trials, `trace_cap`): the
                     decoded xq of the trial (decode_xq is one to one on the parameters a set moves) and its error
  c{c}_sgrproj, c{c}_sse   [units][4] ep, xqd0, xqd1, 0 and [units] sse[RESTORE_SGRPROJ] as search_sgrproj_seg leaves them
  c{c}_fsums         [3][16][4] sum flt0, sum flt0^2, sum flt1, sum flt1^2 over each plane in search geometry (0 for a radius of 0)
  c{c}_fdump         64x64 pictures only: [3 sets `dump_ep`][2] planes of flt - u, the three planes flattened one after the other
  c{c}_ftype, c{c}_utype, c{c}_utaps, c{c}_usgr   [3 runs] frame types, unit types, Wiener taps, SgrprojInfo of each filter run: all units
                     RESTORE_SGRPROJ with the search's result; NONE / WIENER / SGRPROJ mixed with random ep and xqd; luma RESTORE_NONE.  In
                     the last two the first unit of each plane carries the extreme xqd of the ranges.
  c{c}_out{r}_d{p}   what av1_loop_restoration_filter_frame left of plane p in run r, minus the CDEF'd plane (absent: frame type NONE)
Constructed cases answered by the restatement alone (tests/lr_sgr_util.py), marked `synthetic`:
  syn_sums, syn_size, syn_ep, syn_xq, syn_xqd, syn_fused_differs   sums for the solve: near-singular ones, of which `syn_fused_differs`
                     marks the rows whose xq changes when Det and x are evaluated with fused multiply-adds (emulated in exact fractions;
                     bit 0: fma(a, b, -(c d)), bit 1: fma(-c, d, a b); at least 5 rows of each asserted), rows with Det < 1e-8 and rows
                     that hit every clamp of encode_xq
  syn_walk_coef, syn_walk_quant, syn_walk_ep, syn_walk_start, syn_walk_xqd, syn_walk_err, syn_walk_ntrials   error tables for the walk,
                     err[x0][x1] = 1000 + (sum_p a_p (x_p - t_p)^2 + b_p |x_p - t_p|) // quant * quant, and what the walk makes of them
Leaf functions: setup_rtcd_internal(ASM_AVX2) as the encoder (av1_selfguided_restoration_avx2, apply_selfguided_restoration_avx2,
get_proj_subspace_avx2, av1_[lowbd|highbd]_pixel_proj_error_avx2); tests/lr_sgr_util.py restates the C forms, so every equality with this
fixture is also a check of C against AVX2.
Coverage: counted by the restatement while it reproduces the reference's run trial by trial; arms the pictures do not reach are listed in
`unreached` and must be reached by the synthetic cases (asserted here and by tests/test_lr_sgr_vs_ref.py::test_fixture_covers_the_ground)."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import lr_sgr_util as su  # noqa: E402
import lr_util as lu  # noqa: E402
import make_golden_lr as mg  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

OUT = os.path.join(HERE, "lr_sgr.npz")
LR_CASES = (0, 1, 2, 4, 5, 6, -1, -1)
EXTRA = {6: (64, 64, 8), 7: (64, 64, 10)}
DUMP_EP = (0, 12, 15)
TRACE_CAP = 48


def build_driver(out_dir):
    """ref_lr_sgr_driver.c, which includes ref_lr_driver.c, by the recipe of oracle/ref_driver.py, with EbRestorationPick.o left out."""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_lr_sgr_driver.c"), out_dir, leave_out=("EbRestorationPick.o",), include=(HERE,))
    L.drv_lr_open.argtypes = [C.c_int] * 3 + [C.c_void_p] * 4
    L.drv_lr_units.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.drv_sgr_search.argtypes = [C.c_int] + [C.c_void_p] * 8
    L.drv_sgr_filter.argtypes = [C.c_void_p] * 6
    L.drv_sgr_time.restype = C.c_double
    L.drv_sgr_time.argtypes = []
    return L


def reference_search(R, n_units, want_dump):
    """per plane what drv_sgr_search notes"""
    res = []
    for p in range(3):
        n = n_units[p]
        ph, pw = R.h >> (p > 0), R.w >> (p > 0)
        r = {"detail": np.zeros((n, 16), su.DETAIL_DTYPE), "sgrproj": np.zeros((n, 4), np.int32), "sse": np.zeros(n, np.int64),
             "trace_xq": np.zeros((n, 16, TRACE_CAP, 2), np.int32), "trace_err": np.zeros((n, 16, TRACE_CAP), np.int64),
             "fsums": np.zeros((16, 4), np.int64), "dump": np.zeros((3, 2, ph, pw), np.int32) if want_dump else None}
        ep = np.array(DUMP_EP, np.int32)
        cap = R.L.drv_sgr_search(p, r["detail"].ctypes.data, r["sgrproj"].ctypes.data, r["sse"].ctypes.data, r["trace_xq"].ctypes.data,
                                 r["trace_err"].ctypes.data, r["fsums"].ctypes.data, ep.ctypes.data, r["dump"].ctypes.data if want_dump else None)
        assert cap == TRACE_CAP
        res.append(r)
    return res


def reference_filter(R, ftype, base, utype, utaps, usgr):
    dt = np.uint16 if R.bd > 8 else np.uint8
    out = [np.zeros((R.h >> (p > 0), R.w >> (p > 0)), dt) for p in range(3)]
    ft, bs = np.array(ftype, np.int32), np.array(base[:3], np.int32)
    ut, tp, sg = np.ascontiguousarray(utype, np.uint8), np.ascontiguousarray(utaps, np.int16), np.ascontiguousarray(usgr, np.int32)
    assert R.L.drv_sgr_filter(ft.ctypes.data, bs.ctypes.data, ut.ctypes.data, tp.ctypes.data, sg.ctypes.data, mg._ptrs(out)) == 0
    return out


def extra_pictures(rng, w, h, bd):
    cdef, dbk, src = mg.make_pictures(rng, w, h, bd)
    cdef[1][:] = 128 if bd == 8 else 514
    cdef[2] = src[2].copy()
    return cdef, dbk, src


def filter_runs(rng, n_units, base, sgrproj):
    taps = np.zeros((n_units, 16), np.int16)
    rnd = np.zeros((n_units, 4), np.int32)
    for u in range(n_units):
        chroma = u >= base[1]
        six = [0 if (chroma and p == 0) else int(rng.integers(lu.TAP_MIN[p], lu.TAP_MAX[p] + 1)) for p in (0, 1, 2, 0, 1, 2)]
        a, b = mg.taps_of(six)
        taps[u] = a + b
        rnd[u] = (int(rng.integers(0, 16)), int(rng.integers(su.PRJ_MIN[0], su.PRJ_MAX[0] + 1)), int(rng.integers(su.PRJ_MIN[1], su.PRJ_MAX[1] + 1)), 0)
    ext1, ext2 = rnd.copy(), rnd.copy()
    for k, b in enumerate(base[:3]):
        ext1[b] = ((3, 12, 15)[k], su.PRJ_MIN[0], su.PRJ_MIN[1], 0)      # xq1 = 128 + 96 + 32: the sharpest
        ext2[b] = ((15, 0, 10)[k], su.PRJ_MAX[0], su.PRJ_MAX[1], 0)
    mixed = rng.integers(0, 3, n_units).astype(np.uint8)
    mixed[base[0]], mixed[base[1]], mixed[base[2]] = 2, 2, 2
    if n_units > 3:
        mixed[1], mixed[n_units - 1] = 1, 0
    two = np.full(n_units, 2, np.uint8)
    return [((1, 1, 1), two, taps, sgrproj.astype(np.int32)), ((1, 1, 1), mixed, taps, ext1), ((0, 1, 1), two, taps, ext2)]


def synthetic_solve(rng):
    """rows (sums[5], size, ep); the near-singular ones first"""
    rows = []
    found = [0, 0]
    for _ in range(200000):
        if min(found) >= 6:
            break
        a, b = int(rng.integers(50, 3000)), int(rng.integers(50, 3000))
        n = int(rng.integers(64, 147456))
        k = int(rng.integers(1, 2000))
        H00, H11 = a * a * k + int(rng.integers(0, 7)), b * b * k + int(rng.integers(0, 7))
        H01 = a * b * k - int(rng.integers(0, 3))
        cc = int(rng.integers(-1000, 1000))                   # C nearly parallel to H's columns: x stays moderate although Det is tiny
        sums = [H00, H11, H01, a * cc * k + int(rng.integers(-3, 4)), b * cc * k + int(rng.integers(-3, 4))]
        ep = int(rng.integers(0, 10))
        xq = su.solve(sums, n, ep)[0]
        if max(abs(v) for v in xq) >= 1 << 20:                # (int32_t)rint(x) must stay defined
            continue
        m = su.fused_mask(sums, n, ep, xq)
        if (m & 1 and found[0] < 6) or (m & 2 and found[1] < 6) or len(rows) < 4:
            rows.append((sums, n, ep))
            found[0] += m & 1
            found[1] += m >> 1
    n_near = len(rows)
    # Det < 1e-8: nothing filtered; a negative determinant; the one-filter arms with an empty H
    rows += [([0, 0, 0, 0, 0], 4096, 3), ([4, 4, 5, 7, 9], 4096, 0), ([9, 0, 0, 5, 0], 1024, 12), ([0, 9, 0, 0, 5], 1024, 15),
             ([0, 0, 0, 0, 0], 1024, 11), ([0, 0, 0, 0, 0], 1024, 14)]
    # every clamp of encode_xq: xqd0 low and high (two-filter and r1 == 0 arms), xqd1 low and high in each of the three arms
    rows += [([100, 100, 0, 500, 0], 64, 0), ([100, 100, 0, -500, 0], 64, 0), ([100, 100, 0, 0, 500], 64, 1), ([100, 100, 0, 0, -500], 64, 1),
             ([100, 0, 0, 500, 0], 64, 14), ([100, 0, 0, -500, 0], 64, 15), ([0, 100, 0, 0, 500], 64, 10), ([0, 100, 0, 0, -100], 64, 13),
             ([100, 100, 0, 25, 100], 64, 5), ([0, 100, 0, 0, 75], 64, 12), ([100, 0, 0, 10, 0], 64, 14)]
    return rows, n_near


def walk_table(coef, quant):
    """err[x0 - MIN0][x1 - MIN1] of a constructed error function"""
    x0 = np.arange(su.PRJ_MIN[0], su.PRJ_MAX[0] + 1, dtype=np.int64)[:, None]
    x1 = np.arange(su.PRJ_MIN[1], su.PRJ_MAX[1] + 1, dtype=np.int64)[None, :]
    e = coef[0][0] * (x0 - coef[0][1]) ** 2 + coef[0][2] * np.abs(x0 - coef[0][1]) + coef[1][0] * (x1 - coef[1][1]) ** 2 + coef[1][2] * np.abs(x1 - coef[1][1])
    return 1000 + e // int(quant) * int(quant)


def synthetic_walks(rng):
    rows = []
    for k in range(18):
        ep = (0, 12, 15, 4, 9, 10)[k % 6]
        coef = np.zeros((2, 3), np.int64)
        start = [0, 0]
        for p in range(2):
            target = (su.PRJ_MIN[p] - 5, su.PRJ_MAX[p] + 5, int(rng.integers(su.PRJ_MIN[p], su.PRJ_MAX[p] + 1)))[(k + p) % 3]
            coef[p] = (int(rng.integers(1, 40)), target, int(rng.integers(0, 30)))
            start[p] = int(rng.integers(su.PRJ_MIN[p], su.PRJ_MAX[p] + 1))
            if k >= 12:                                  # close to an end: the range stops
                start[p] = (su.PRJ_MIN[p] + k % 2, su.PRJ_MAX[p] - k % 2)[(k + p) % 2]
        quant = (1, 16, 1 << 30)[k % 3]                  # the last: every trial ties
        rows.append((coef, quant, ep, start))
    return rows


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    rng = np.random.default_rng(20261019)
    lrz = dict(np.load(os.path.join(HERE, "lr.npz")))
    out = {"lr_case": np.array(LR_CASES, np.int32), "dump_ep": np.array(DUMP_EP, np.int32), "trace_cap": np.array(TRACE_CAP, np.int32)}
    st_box, st_walk, st_flt = su.new_box_stats(), su.new_walk_stats(), su.new_filter_stats()
    best_tie = False
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for c, lc in enumerate(LR_CASES):
            if lc >= 0:
                F = lu.load_case(lrz, lc)
                w, h, bd, cdef, dbk, src = F["w"], F["h"], F["bd"], F["cdef"], F["dbk"], F["src"]
            else:
                w, h, bd = EXTRA[c]
                cdef, dbk, src = extra_pictures(rng, w, h, bd)
                for p in range(3):
                    out[f"x{c}_src_{p}"] = src[p]
                    out[f"x{c}_dbk_d{p}"], out[f"x{c}_cdef_d{p}"] = mg.delta(dbk[p], src[p]), mg.delta(cdef[p], dbk[p])
                out[f"x{c}_size"] = np.array([w, h, bd], np.int32)
            R = mg.Reference(L, w, h, bd, cdef, dbk, src)
            limits, _ = R.units()
            planes, base = lu.picture_units(w, h)
            for p in range(3):
                assert np.array_equal(limits[p], planes[p][0])
            n_units = [len(v) for v in limits]
            small = w == 64
            res = reference_search(R, n_units, small)
            cat = lambda k: np.concatenate([r[k] for r in res])  # noqa: E731
            detail, sgrproj, sse = cat("detail"), cat("sgrproj"), cat("sse")
            txq, terr = cat("trace_xq"), cat("trace_err")
            # the restatement reproduces the reference's run; coverage is counted on the way
            tq, te = [], []
            for p in range(3):
                ss = int(p > 0)
                for i, lim in enumerate(planes[p][0]):
                    u = base[p] + i
                    det, traces, best = su.search_unit(cdef[p], src[p], lim, bd, ss, st_box, st_walk)
                    for k in det.dtype.names:
                        assert np.array_equal(det[k], detail[u][k]), ("the restatement's search differs from the reference's", c, u, k, det[k], detail[u][k])
                    assert list(best) == [int(v) for v in sgrproj[u][:3]], (c, u, best, sgrproj[u])
                    errs = [int(e) for e in det["err"]]
                    best_tie |= errs.count(min(errs)) > 1
                    assert su.trial_sse(cdef[p], dbk[p], src[p], lim, best[0], best[1:], bd, ss, st_flt) == int(sse[u]), (c, u)
                    for ep in range(16):
                        nt = min(len(traces[ep]), TRACE_CAP)
                        mine_xq = [su.decode_xq(q, ep) for (q, _) in traces[ep][:nt]]
                        assert mine_xq == [[int(v) for v in row] for row in txq[u, ep, :nt]], (c, u, ep)
                        assert [e for (_, e) in traces[ep][:nt]] == [int(v) for v in terr[u, ep, :nt]], (c, u, ep)
                        tq.append(txq[u, ep, :nt]), te.append(terr[u, ep, :nt])
            out[f"c{c}_detail"], out[f"c{c}_sgrproj"], out[f"c{c}_sse"] = detail, sgrproj, sse
            out[f"c{c}_trace_xq"], out[f"c{c}_trace_err"] = np.concatenate(tq).astype(np.int16), np.concatenate(te)
            out[f"c{c}_fsums"] = np.array([r["fsums"] for r in res])
            for p in range(3):
                for ep in range(16):
                    flt = su.plane_flt(cdef[p], planes[p][0], bd, ep, int(p > 0))
                    mine = [v for k in range(2) for v in ((int(flt[k].sum()), int((flt[k] * flt[k]).sum())) if flt[k] is not None else (0, 0))]
                    assert mine == [int(v) for v in res[p]["fsums"][ep]], (c, p, ep, mine, res[p]["fsums"][ep])
            if small:
                out[f"c{c}_fdump"] = np.concatenate([r["dump"].reshape(3, 2, -1) for r in res], axis=2).astype(np.int16)
                assert all(np.abs(r["dump"]).max() < 32768 for r in res)
            runs = filter_runs(rng, sum(n_units), base, sgrproj)
            out[f"c{c}_ftype"] = np.array([r[0] for r in runs], np.int32)
            out[f"c{c}_utype"] = np.array([r[1] for r in runs], np.uint8)
            out[f"c{c}_utaps"] = np.array([r[2] for r in runs], np.int16)
            out[f"c{c}_usgr"] = np.array([r[3] for r in runs], np.int32)
            for r, (ft, ut, tp, sg) in enumerate(runs):
                got = reference_filter(R, ft, base, ut, tp, sg)
                mine_out = su.filter_frame(cdef, dbk, w, h, bd, ft, ut, tp, sg, st_flt)
                for p in range(3):
                    assert np.array_equal(got[p], mine_out[p]), ("the restatement's frame filter differs from the reference's", c, r, p)
                    if ft[p]:
                        out[f"c{c}_out{r}_d{p}"] = mg.delta(got[p], cdef[p])
            R.close()
            print("case", c, (w, h, bd), "units", n_units, "best", [[int(v) for v in s[:3]] for s in sgrproj], "trials/(unit, ep)",
                  round(float(detail["n_trials"].mean()), 2), "max", int(detail["n_trials"].max()))
            assert int(detail["n_trials"].max()) <= su.max_walk_trials()
    reached = {**st_box, **{k: v for k, v in st_flt.items() if k != "neither"}, **st_walk, "best_ep_tie": int(best_tie)}
    unreached = [k for k, v in reached.items() if not v]
    print("reached", reached, "unreached", unreached)
    out["unreached"] = np.array(unreached, dtype="U16")
    # constructed sums for the solve
    rows, n_near = synthetic_solve(rng)
    sol = [su.solve(s, n, ep) for (s, n, ep) in rows]
    fused = [su.fused_mask(s, n, ep, x[0]) for (s, n, ep), x in zip(rows, sol)]
    assert sum(m & 1 for m in fused) >= 5 and sum(m >> 1 for m in fused) >= 5, fused
    xqd = np.array([x[1] for x in sol], np.int32)
    for p in range(2):
        assert (xqd[:, p] == su.PRJ_MIN[p]).any() and (xqd[:, p] == su.PRJ_MAX[p]).any(), ("a clamp of encode_xq is not hit", p)
    out["syn_sums"], out["syn_size"] = np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int32)
    out["syn_ep"], out["syn_xq"], out["syn_xqd"] = np.array([r[2] for r in rows], np.int32), np.array([x[0] for x in sol], np.int32), xqd
    out["syn_fused_differs"] = np.array(fused, np.uint8)
    # constructed error tables for the walk
    sw = su.new_walk_stats()
    syn = synthetic_walks(rng)
    fin, errs, ntr = [], [], []
    for (coef, quant, ep, start) in syn:
        T = walk_table(coef, quant)
        e, q, trace = su.walk(lambda x: int(T[x[0] - su.PRJ_MIN[0], x[1] - su.PRJ_MIN[1]]), start, ep, sw)
        fin.append(q), errs.append(e), ntr.append(len(trace))
        assert len(trace) <= su.max_walk_trials()
    assert all(sw.values()), sw
    assert all(k in sw for k in unreached if k in st_walk)
    assert not [k for k in unreached if k not in sw], ("not reached by the pictures and not by a synthetic case", unreached)
    out["syn_walk_coef"], out["syn_walk_quant"] = np.array([s[0] for s in syn]), np.array([s[1] for s in syn], np.int64)
    out["syn_walk_ep"], out["syn_walk_start"] = np.array([s[2] for s in syn], np.int32), np.array([s[3] for s in syn], np.int32)
    out["syn_walk_xqd"], out["syn_walk_err"], out["syn_walk_ntrials"] = np.array(fin, np.int32), np.array(errs, np.int64), np.array(ntr, np.int32)
    np.savez_compressed(OUT, **out)
    mg.print_sizes(out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
