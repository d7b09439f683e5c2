"""Writes tests/golden/lr.npz from the reference's own Wiener restoration search and frame filter (tests/golden/ref_lr_driver.c, which is
the reference's EbRestorationPick.c included where it lies plus calls, linked against the reference objects of the oracle build,
oracle/_ref/obj_all, in place of EbRestorationPick.o).  Run in the build container only, where the reference exists: the fixture is data.

    python tests/golden/make_golden_lr.py

Pictures are synthetic: the source is smooth texture plus edges (some saturated), the deblocked picture the source blurred and coarsely
quantised, the CDEF'd picture the deblocked one changed again so that substituted stripe rows differ from the rows they replace.
Contents, per case c (`case` holds width, height, bit depth per row; 64x64, 200x136, 136x200, 392x264 at 8 bits, the first three at 10:
the 10-bit run of the largest picture is left out to keep the file within the limit for a committed file)
  c{c}_src_{p}, c{c}_dbk_d{p}, c{c}_cdef_d{p}  the source planes; deblocked - source; CDEF'd - deblocked (lr_util.load_case adds them up)
  c{c}_unit_size, c{c}_base                   unit size per plane; index of each plane's first unit in the per-unit arrays
  c{c}_limits                                 [units][4] h_start, h_end, v_start, v_end as av1_foreach_rest_unit_in_frame hands them out
  c{c}_M, c{c}_avg                            [units][49] (the first win^2 entries used), [units]
  c{c}_Hu                                     the upper triangles of H, row after row, unit after unit (lr_util.load_case expands them to
                                              [units][49*49], of which the first win^4 entries are used; the reference mirrors H itself)
  c{c}_start, c{c}_rejected                   [units][16] vfilter[8] + hfilter[8] after finalize_sym_filter; compute_score > 0
  c{c}_sse                                    [units][2] sse[RESTORE_NONE], sse[RESTORE_WIENER] (INT64_MAX when rejected)
  c{c}_final, c{c}_n_trials                   [units][16] the taps search_wiener_seg left (zeros when rejected); number of trial filters
  c{c}_trace_taps, c{c}_trace_sse             all trials of all units in order, unit after unit (split by n_trials): taps, SSE
  c{c}_ftype, c{c}_utype, c{c}_utaps          [runs][3] frame types, [runs][units] unit types, [runs][units][16] taps of each filter run
  c{c}_out{r}_d{p}                            what av1_loop_restoration_filter_frame left of plane p in run r, minus the CDEF'd plane; absent
                                              for a plane whose frame type is RESTORE_NONE, which the reference leaves as it is
Constructed cases answered by the restatement alone (tests/lr_util.py), marked `synthetic`:
  syn_walk_coef, syn_walk_start, syn_walk_win  error functions err = sum_i coef[i][0] * (tap_i - coef[i][1])^2 + coef[i][2] * |..| over the
                                              six free taps (v0..v2, h0..h2), quantised by syn_walk_quant to make ties
  syn_walk_ntrials, syn_walk_final, syn_walk_err   what the walk makes of them
  syn_M, syn_H, syn_win, syn_start, syn_rejected   constructed M and H for the solver (scaled and perturbed statistics)
Leaf functions: setup_rtcd_internal(ASM_AVX2) as the encoder, so av1_compute_stats[_highbd]_avx2, av1_[highbd_]wiener_convolve_add_src_avx2
and aom_mse16x16_avx2; tests/lr_util.py restates the C forms, so every equality with this fixture is also a check of C against AVX2.  The
10-bit SSE's 16x16 leaf is NASM code the link lacks; the driver's stand-in has its contract.
Coverage: coverage() below, asserted again by tests/test_lr_vs_ref.py::test_fixture_covers_the_ground.  Arms the pictures do not reach are
listed in `unreached` (names of lr_util's statistics) and are covered by the synthetic cases."""
import ctypes as C
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import lr_util as lu  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

OUT = os.path.join(HERE, "lr.npz")
CASES = ((64, 64, 8), (200, 136, 8), (136, 200, 8), (392, 264, 8), (64, 64, 10), (200, 136, 10), (136, 200, 10))
TRACE_CAP = 128


def build_driver(out_dir):
    """ref_lr_driver.c by the recipe of oracle/ref_driver.py, with EbRestorationPick.o left out: the driver is that file."""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_lr_driver.c"), out_dir, leave_out=("EbRestorationPick.o",))
    L.drv_lr_open.argtypes = [C.c_int] * 3 + [C.c_void_p] * 4
    L.drv_lr_units.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.drv_lr_search.argtypes = [C.c_int] + [C.c_void_p] * 10
    L.drv_lr_filter.argtypes = [C.c_void_p] * 5
    L.drv_lr_time.restype = C.c_double
    L.drv_lr_time.argtypes = [C.c_void_p]
    return L


def _ptrs(planes):
    return (C.c_void_p * 3)(*[p.ctypes.data for p in planes])


class Reference:
    """one opened picture in the driver"""

    def __init__(self, L, w, h, bd, cdef, dbk, src):
        self.L, self.w, self.h, self.bd = L, w, h, bd
        self.unit = np.array(lu.unit_sizes(w, h), np.int32)
        self.keep = [np.ascontiguousarray(p) for s in (cdef, dbk, src) for p in s]
        assert L.drv_lr_open(w, h, bd, self.unit.ctypes.data, _ptrs(self.keep[0:3]), _ptrs(self.keep[3:6]), _ptrs(self.keep[6:9])) == 0

    def close(self):
        self.L.drv_lr_close()

    def units(self):
        out, horz = [], []
        for p in range(3):
            lim, hz = np.zeros((64, 4), np.int32), np.zeros(1, np.int32)
            n = self.L.drv_lr_units(p, lim.ctypes.data, hz.ctypes.data)
            out.append(lim[:n].copy()), horz.append(int(hz[0]))
        return out, horz

    def search(self, n_units):
        res = []
        for p in range(3):
            n = n_units[p]
            r = {"M": np.zeros((n, 49), np.int64), "H": np.zeros((n, 2401), np.int64), "avg": np.zeros(n, np.int32), "rejected": np.zeros(n, np.int32),
                 "start": np.zeros((n, 16), np.int16), "sse": np.zeros((n, 2), np.int64), "final": np.zeros((n, 16), np.int16),
                 "n_trials": np.zeros(n, np.int32), "trace_taps": np.zeros((n, TRACE_CAP, 16), np.int16), "trace_sse": np.zeros((n, TRACE_CAP), np.int64)}
            cap = self.L.drv_lr_search(p, *[r[k].ctypes.data for k in ("M", "H", "avg", "rejected", "start", "sse", "final", "n_trials", "trace_taps",
                                                                       "trace_sse")])
            assert cap == TRACE_CAP and int(r["n_trials"].max(initial=0)) <= TRACE_CAP
            res.append(r)
        return res

    def filter_frame(self, ftype, base, utype, utaps):
        dt = np.uint16 if self.bd > 8 else np.uint8
        out = [np.zeros((self.h >> (p > 0), self.w >> (p > 0)), dt) for p in range(3)]
        ft, bs = np.array(ftype, np.int32), np.array(base[:3], np.int32)
        ut, tp = np.ascontiguousarray(utype, np.uint8), np.ascontiguousarray(utaps, np.int16)
        assert self.L.drv_lr_filter(ft.ctypes.data, bs.ctypes.data, ut.ctypes.data, tp.ctypes.data, _ptrs(out)) == 0
        return out


def delta(a, b):
    """a - b as int16 (int8 where it fits): the planes differ little from each other, so the differences compress"""
    d = a.astype(np.int32) - b.astype(np.int32)
    return d.astype(np.int8 if np.abs(d).max(initial=0) < 128 else np.int16)


def print_sizes(out):
    """the eight largest groups of arrays by compressed size, the per-case arrays c{c}_* / x{c}_* of one name taken together"""
    sizes = {}
    for k, v in out.items():
        bio = io.BytesIO()
        np.savez_compressed(bio, a=v)
        g = k.split("_", 1)[1].rstrip("0123456789") if k[0] in "cx" and k[1].isdigit() else k
        sizes[g] = sizes.get(g, 0) + bio.getbuffer().nbytes
    print(sorted(sizes.items(), key=lambda kv: -kv[1])[:8])


def make_pictures(rng, w, h, bd):
    """source, deblocked, CDEF'd planes: low-entropy constructions so that the fixture compresses"""
    top = (1 << bd) - 1
    sh = bd - 8
    src, dbk, cdef = [], [], []
    for p in range(3):
        pw, ph = w >> (p > 0), h >> (p > 0)
        y, x = np.mgrid[0:ph, 0:pw]
        f = 110 + 60 * np.sin(x / (5.0 + 2 * p)) * np.cos(y / (7.0 + p)) + 0.3 * x - 0.2 * y
        f += 50 * ((x // 24 + y // 20) % 2)                        # edges
        f += 10 * np.sin(x * (1.3 + 0.2 * p) + y * 0.9)            # fine texture
        for _ in range(3):                                         # saturated patches, black and white
            cx, cy, v = rng.integers(0, pw), rng.integers(0, ph), rng.integers(0, 2)
            f[max(cy - 6, 0):cy + 6, max(cx - 9, 0):cx + 9] = 400 * v - 100
            f[max(cy - 6, 0):cy + 6, cx:cx + 1] = 300 - 400 * v    # a one-sample line of the other extreme: drives the horizontal clamps
        s = np.clip(np.round(f / 4) * 4, 0, 255).astype(np.int64) << sh
        pad = np.pad(s, 2, mode="edge")
        blur = sum(pad[dy:dy + ph, dx:dx + pw] * wgt for dy, dx, wgt in ((2, 2, 4), (2, 0, 1), (2, 4, 1), (0, 2, 1), (4, 2, 1), (2, 1, 2), (2, 3, 2),
                                                                        (1, 2, 2), (3, 2, 2))) // 16
        q = 4 << sh
        d = np.clip((blur + (q >> 1)) // q * q + ((x * 3 + y * 5) % 7 - 3) // 3 * (1 << sh), 0, top)
        d[s == 0], d[s == (255 << sh)] = 0, top                    # saturated stays saturated: drives the clips
        c = np.clip(d + ((x * 7 + y * 3) % 5 - 2) * (2 << sh) * ((x + y) % 3 == 0), 0, top)
        c[s == 0], c[s == (255 << sh)] = 0, top
        if p == 2 and w == 64:                                     # next to no degradation: the learned filter cannot beat the identity
            c = np.clip(s + ((x * 5 + y * 3) % 11 == 0), 0, top)
        dt = np.uint16 if bd > 8 else np.uint8
        src.append(s.astype(dt)), dbk.append(d.astype(dt)), cdef.append(c.astype(dt))
    return cdef, dbk, src


def synthetic_walks(rng):
    rows = []
    for win in (7, 5):
        off = (7 - win) >> 1
        for k in range(12):
            coef = np.zeros((6, 3), np.int64)
            for i in range(6):
                p = i % 3
                target = (lu.TAP_MIN[p] - 3, lu.TAP_MAX[p] + 3, lu.TAP_MID[p], int(rng.integers(lu.TAP_MIN[p], lu.TAP_MAX[p] + 1)))[(k + i) % 4]
                coef[i] = (int(rng.integers(0, 50)), target, int(rng.integers(0, 30)))
            start = [0 if p < off else int(rng.integers(lu.TAP_MIN[p], lu.TAP_MAX[p] + 1)) for p in (0, 1, 2, 0, 1, 2)]
            quant = (1, 64, 1 << 20)[k % 3]        # the last: every trial ties
            rows.append((coef, np.array(start, np.int16), win, quant))
    return rows


def synthetic_error(coef, quant):
    def err(vf, hf):
        t = [int(v) for v in vf[:3]] + [int(v) for v in hf[:3]]
        e = sum(int(c[0]) * (t[i] - int(c[1])) ** 2 + int(c[2]) * abs(t[i] - int(c[1])) for i, c in enumerate(coef))
        return 1000000 + e // quant * quant
    return err


def taps_of(start6):
    v, h = [int(t) for t in start6[:3]], [int(t) for t in start6[3:]]
    return (v + [-2 * sum(v)] + v[::-1] + [0]), (h + [-2 * sum(h)] + h[::-1] + [0])


def restatement_of_case(w, h, bd, cdef, dbk, src, st_f, st_w):
    """the restatement's own search of every unit, for the coverage statistics: [(rejected, n_trials)]"""
    planes, base = lu.picture_units(w, h)
    res = []
    for p in range(3):
        win, ss = (7, 5)[p > 0], int(p > 0)
        for lim in planes[p][0]:
            M, H, _ = lu.compute_stats(cdef[p], src[p], lim, win, bd)
            vf, hf, rej = lu.solve(M, H, win)
            n = 0
            if not rej:
                _, _, _, trace = lu.walk(lambda a, b: lu.trial_sse(cdef[p], dbk[p], src[p], lim, a, b, bd, ss, st_f), vf, hf, win, st_w)
                n = len(trace)
            res.append((rej, n))
    return res


def coverage(geometry, st_f, st_w, rejected):
    """what of the issue's list the reference's recorded run does not reach (names), from statistics counted on its own trials"""
    missing = [k for k in ("above_only", "below_only", "both", "clamp_lo", "clamp_hi", "clip_lo", "clip_hi") if not st_f[k]]
    missing += [k for k in ("minus", "plus", "repeat", "skip_break", "tie", "range_stop") if not st_w[k]]
    missing += [k for k, v in geometry.items() if not v]
    if not rejected:
        missing.append("rejected")
    return missing


def geometry_coverage(cases):
    g = {"early_start": False, "early_end": False, "wide_remainder": False}
    for (w, h, bd) in cases:
        planes, _ = lu.picture_units(w, h)
        unit = lu.unit_sizes(w, h)
        for p in range(3):
            ph, off = h >> (p > 0), 8 >> (p > 0)
            for (h0, h1, v0, v1) in planes[p][0]:
                g["early_start"] |= v0 > 0 and (v0 + off) % unit[p] == 0
                g["early_end"] |= v1 < ph
                g["wide_remainder"] |= (h1 - h0) > unit[p] or (v1 - v0) > unit[p]
    return g


def filter_runs(rng, n_units, base, final, rejected):
    """frame types, unit types, taps per run: all Wiener with the search's taps (default taps where rejected); mixed types with random
    taps; luma RESTORE_NONE.  In the last two the first unit of each plane has the sharpest taps the ranges allow (clamps and clips)."""
    default = np.array(taps_of(lu.TAP_MID * 2)[0] + taps_of(lu.TAP_MID * 2)[1], np.int16)
    taps = np.where(rejected[:, None] != 0, default[None, :], final).astype(np.int16)
    rnd = taps.copy()
    for u in range(n_units):
        chroma = u >= base[1]
        six = [0 if (chroma and p == 0) else int(rng.integers(lu.TAP_MIN[p], lu.TAP_MAX[p] + 1)) for p in (0, 1, 2, 0, 1, 2)]
        if u in base[:3]:
            six = [0 if (chroma and p == 0) else lu.TAP_MIN[p] for p in (0, 1, 2, 0, 1, 2)]
        if chroma:
            taps[u, [0, 6, 8, 14]] = 0
            taps[u, 3], taps[u, 11] = -2 * (taps[u, 1] + taps[u, 2]), -2 * (taps[u, 9] + taps[u, 10])
        a, b = taps_of(six)
        rnd[u] = a + b
    mixed = rng.integers(0, 2, n_units).astype(np.uint8)
    mixed[base[0]], mixed[base[1]], mixed[base[2]] = 1, 1, 0      # both types in every run, also with one unit per plane
    if n_units > 3:
        mixed[1], mixed[n_units - 1] = 0, 1
    return [((1, 1, 1), np.ones(n_units, np.uint8), taps), ((1, 1, 1), mixed, rnd), ((0, 1, 1), np.ones(n_units, np.uint8), rnd)]


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    rng = np.random.default_rng(20261018)
    out = {"case": np.array(CASES, np.int32)}
    st_f, st_w, any_rejected = lu.new_filter_stats(), lu.new_walk_stats(), False
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for c, (w, h, bd) in enumerate(CASES):
            cdef, dbk, src = make_pictures(rng, w, h, bd)
            R = Reference(L, w, h, bd, cdef, dbk, src)
            limits, horz = R.units()
            planes, base = lu.picture_units(w, h)
            for p in range(3):
                assert np.array_equal(limits[p], planes[p][0]) and horz[p] == planes[p][1], ("geometry differs from the reference's", c, p)
            n_units = [len(v) for v in limits]
            res = R.search(n_units)
            cat = lambda k: np.concatenate([r[k] for r in res])  # noqa: E731
            ntr = cat("n_trials")
            tt = np.concatenate([r["trace_taps"][u, :r["n_trials"][u]] for r in res for u in range(len(r["n_trials"]))] or [np.zeros((0, 16), np.int16)])
            ts = np.concatenate([r["trace_sse"][u, :r["n_trials"][u]] for r in res for u in range(len(r["n_trials"]))] or [np.zeros(0, np.int64)])
            for p in range(3):
                out[f"c{c}_src_{p}"] = src[p]
                out[f"c{c}_dbk_d{p}"], out[f"c{c}_cdef_d{p}"] = delta(dbk[p], src[p]), delta(cdef[p], dbk[p])
            out[f"c{c}_unit_size"], out[f"c{c}_base"] = R.unit, np.array(base, np.int32)
            out[f"c{c}_limits"] = np.concatenate(limits)
            for k in ("M", "avg", "start", "rejected", "sse", "final"):
                out[f"c{c}_{k}"] = cat(k)
            out[f"c{c}_Hu"] = np.concatenate([lu.pack_upper(r["H"][u], (7, 5)[p > 0]) for p, r in enumerate(res) for u in range(len(r["H"]))])
            out[f"c{c}_n_trials"], out[f"c{c}_trace_taps"], out[f"c{c}_trace_sse"] = ntr, tt, ts
            runs = filter_runs(rng, sum(n_units), base, cat("final"), cat("rejected"))
            out[f"c{c}_ftype"] = np.array([r[0] for r in runs], np.int32)
            out[f"c{c}_utype"] = np.array([r[1] for r in runs], np.uint8)
            out[f"c{c}_utaps"] = np.array([r[2] for r in runs], np.int16)
            for r, (ft, ut, tp) in enumerate(runs):
                got = R.filter_frame(ft, base, ut, tp)
                mine_out = lu.filter_frame(cdef, dbk, w, h, bd, ft, ut, tp, st=st_f)
                for p in range(3):
                    assert np.array_equal(got[p], mine_out[p]), ("the restatement's frame filter differs from the reference's", c, r, p)
                    if ft[p]:
                        out[f"c{c}_out{r}_d{p}"] = delta(got[p], cdef[p])
                    else:
                        assert np.array_equal(got[p], cdef[p])
            R.close()
            # coverage, counted on the reference's own trials: the restatement must have run the same ones
            mine = restatement_of_case(w, h, bd, cdef, dbk, src, st_f, st_w)
            assert [m[1] for m in mine] == [int(v) for v in ntr], ("the restatement ran other trials than the reference", c, mine, ntr)
            any_rejected |= bool(cat("rejected").any())
            print("case", c, (w, h, bd), "units", n_units, "trials", [int(v) for v in ntr], "rejected", [int(v) for v in cat("rejected")])
    unreached = coverage(geometry_coverage(CASES), st_f, st_w, any_rejected)
    print("filter", st_f, "walk", st_w, "unreached", unreached)
    out["unreached"] = np.array(unreached, dtype="U16")
    # constructed walks
    syn = synthetic_walks(rng)
    sw = lu.new_walk_stats()
    fin, ntr, errs = [], [], []
    for (coef, start, win, quant) in syn:
        vf, hf = taps_of(start)
        e, v, hh, trace = lu.walk(synthetic_error(coef, quant), vf, hf, win, sw)
        fin.append(v + hh), ntr.append(len(trace)), errs.append(e)
    assert all(sw.values()), sw
    out["syn_walk_coef"], out["syn_walk_start"] = np.array([s[0] for s in syn]), np.array([s[1] for s in syn])
    out["syn_walk_win"], out["syn_walk_quant"] = np.array([s[2] for s in syn], np.int32), np.array([s[3] for s in syn], np.int64)
    out["syn_walk_final"], out["syn_walk_ntrials"], out["syn_walk_err"] = np.array(fin, np.int16), np.array(ntr, np.int32), np.array(errs, np.int64)
    # constructed statistics for the solver: the first luma and chroma unit of case 1, M scaled / sign-flipped, H perturbed on the diagonal
    sM, sH, sw_, ss_, sr = [], [], [], [], []
    for u, win in ((0, 7), (int(out["c1_base"][1]), 5)):
        M0, H0 = out["c1_M"][u].copy(), lu.load_case(out, 1)["H"][u].copy()
        n = win * win
        for k, (ms, hd) in enumerate(((1, 0), (-1, 0), (3, 0), (1, 5), (0, 0), (-2, 1))):
            M, H = M0 * ms, H0.copy()
            H[:n * n].reshape(n, n)[np.arange(n), np.arange(n)] += hd * (abs(int(H0[0])) // 8)
            if (ms, hd) == (0, 0):
                M[:n] = H[:n * n].reshape(n, n)[n // 2] // 2       # M = half the centre column: the identity scores 0
            vf, hf, rej = lu.solve(M, H, win)
            sM.append(M), sH.append(H), sw_.append(win), ss_.append(vf + hf), sr.append(int(rej))
    assert any(sr) and not all(sr), sr
    out["syn_M"], out["syn_H"], out["syn_win"] = np.array(sM), np.array(sH), np.array(sw_, np.int32)
    out["syn_start"], out["syn_rejected"] = np.array(ss_, np.int16), np.array(sr, np.int32)
    np.savez_compressed(OUT, **out)
    print_sizes(out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
