"""Writes tests/golden/lr_finish.npz from the reference's own rest_finish_search (Codec/EbRestorationPick.c:1971-2040) through
tests/golden/ref_lr_finish_driver.c, built by the recipe of oracle/ref_driver.py.  This file holds no reference text.  Run in the build
container only, where the reference exists: the fixture is data.

    python tests/golden/make_golden_lr_finish.py

Two parts.  The constructed cases of tests/lr_finish_util.constructed_cases: tables only, the reference's unit walk yields the unit counts
from (width, height, unit_size[3]) and rest_finish_search reads no sample.  And the three pictures of tests/golden/post_filter_chain.npz:
the decision on that fixture's own wiener_sse, taps, sgr_sse and sgrproj under at most four settings a picture from the grid
lr_finish_util.CHAIN_RDMULT x CHAIN_X, each with the digest of the reference frame filter's restored planes (the CDEF'd and deblocked
planes come from the reference's chain of make_golden_post_filter_chain.py, checked against that fixture's digests).

The coverage list (lr_finish_util.coverage, and the chain items below) is asserted on the REFERENCE's outputs; the restatement is compared
with the reference on every case and setting, so a restatement that errs stops the generator.

Contents (few arrays: an array costs more in the file than a case's numbers do)
  names, geom, unit_base, rates, range   per constructed case: its name; width, height, unit_size[3]; unit_base[4]; rdmult and the seven
                                     costs; plane_start, plane_end
  wiener_sse, taps, sgr_sse, sgrproj the input tables in the device layouts, the cases' units one after the other
  unit_type, best_rtype              the reference's outputs per unit, likewise
  sse, bits, cost, frame_type, n_tried   [case][3][4] resp. [case][3]: the reference's outputs per plane (all three planes)
  leaf_*                             count_wiener_bits / count_sgrproj_bits alone on a sample of (ref, v) pairs
  {n}_settings                       [k][2] rdmult, X of picture n (A, B, C)
  {n}_unit_type ... {n}_n_tried, {n}_digest_restored   [k][...] the reference's outputs under setting k, film_grain_util.digest of its
                                     restored planes"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import lr_finish_util as fu  # noqa: E402
import lr_util as lu  # noqa: E402
import make_golden_cdef as mg_cdef  # noqa: E402
import make_golden_lr as mg_lr  # noqa: E402
import make_golden_lr_sgr as mg_sgr  # noqa: E402
import make_golden_post_filter_chain as mg_chain  # noqa: E402
import post_filter_chain_util as pc  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

SIZE_LIMIT = 100_000
# the settings the issue names, per picture; the rest of the coverage is filled from the grid
NAMED_SETTINGS = {"A": [(10_000_000, 1 << 22), (60000, 1 << 26)], "B": [(10_000_000, 1 << 22)], "C": [(2_000_000, 1 << 18)]}
MAX_SETTINGS = 4


def build_driver(out_dir):
    """ref_lr_finish_driver.c, which includes ref_lr_sgr_driver.c and through it ref_lr_driver.c, with EbRestorationPick.o left out"""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_lr_finish_driver.c"), out_dir, leave_out=("EbRestorationPick.o",), include=(HERE,))
    L.drv_lr_open.argtypes = [C.c_int] * 3 + [C.c_void_p] * 4
    L.drv_lr_units.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.drv_sgr_filter.argtypes = [C.c_void_p] * 6
    L.drv_finish.argtypes = [C.c_void_p] * 13
    L.drv_finish_bits.argtypes = [C.c_int] + [C.c_void_p] * 7
    L.drv_finish_time.restype = C.c_double
    L.drv_finish_time.argtypes = [C.c_void_p] * 6 + [C.c_int]
    return L


def open_geometry(L, w, h, unit_size):
    """a picture of zeros with this size and these unit sizes: (unit counts of the reference's own unit walk)"""
    us = np.array(unit_size, np.int32)
    planes = [np.zeros((h >> (p > 0), w >> (p > 0)), np.uint8) for p in range(3)]
    assert L.drv_lr_open(w, h, 8, us.ctypes.data, mg_lr._ptrs(planes), mg_lr._ptrs(planes), mg_lr._ptrs(planes)) == 0
    counts = []
    for p in range(3):
        lim, hz = np.zeros((4096, 4), np.int32), np.zeros(1, np.int32)
        counts.append(int(L.drv_lr_units(p, lim.ctypes.data, hz.ctypes.data)))
    return counts


def reference_finish(L, rates, unit_base, wiener_sse, taps, sgr_sse, sgrproj):
    """drv_finish on an open picture: the outputs by the names of lr_finish_util.OUTPUT_KEYS"""
    n = int(unit_base[3])
    ra, ub = fu.rates_array(rates), np.array(unit_base, np.int32)
    ins = [np.ascontiguousarray(a, dt) for a, dt in ((wiener_sse, np.int64), (taps, np.int16), (sgr_sse, np.int64), (sgrproj, np.int32))]
    out = {"unit_type": np.full(n, 0x5A, np.uint8), "frame_type": np.zeros(3, np.int32), "best_rtype": np.full((n, 4), 0x5A, np.uint8),
           "sse": np.zeros((3, 4), np.int64), "bits": np.zeros((3, 4), np.int64), "cost": np.zeros((3, 4), np.float64), "n_tried": np.zeros(3, np.int32)}
    differ = L.drv_finish(ra.ctypes.data, ub.ctypes.data, *[a.ctypes.data for a in ins],
                          *[out[k].ctypes.data for k in ("unit_type", "frame_type", "best_rtype", "sse", "bits", "cost", "n_tried")])
    assert differ == 0, "rest_finish_search and its walks called one by one choose different frame types"
    return out


def reference_bits(L, win, taps, ref, sgr, sgr_ref):
    n = len(win)
    a = [np.ascontiguousarray(v, np.int32) for v in (win, taps, ref, sgr, sgr_ref)]
    wb, sb = np.zeros(n, np.int32), np.zeros(n, np.int32)
    L.drv_finish_bits(n, *[v.ctypes.data for v in a], wb.ctypes.data, sb.ctypes.data)
    return wb, sb


def leaf_sample(rng, n=400):
    win = rng.choice([7, 5], n).astype(np.int32)
    tap = lambda: np.stack([rng.integers(fu.TAP_MIN[j % 3], fu.TAP_MAX[j % 3] + 1, n) for j in range(6)], 1).astype(np.int32)  # noqa: E731
    prj = lambda: np.stack([rng.integers(fu.PRJ_MIN[k], fu.PRJ_MAX[k] + 1, n) for k in range(2)], 1).astype(np.int32)  # noqa: E731
    sgr = np.concatenate([rng.integers(0, 16, (n, 1)).astype(np.int32), prj()], 1)
    return win, tap(), tap(), sgr, prj()


def check_restatement(want, rates, unit_base, tables, what):
    mine = fu.finish(rates, unit_base, *tables)
    diff = fu.first_difference(mine, want)
    assert diff is None, f"{what}: the restatement differs from the reference at {diff}"


def chain_part(L, D, out):
    """the decisions of the chain pictures and the reference frame filter's digests; returns coverage facts"""
    grid = [(rm, x) for rm in fu.CHAIN_RDMULT for x in fu.CHAIN_X]
    results, opened = {}, {}
    for name, P in pc.PICTURES.items():
        mi, recon, source = pc.make_picture(name)
        want = pc.expected(name, recon)
        ref = mg_chain.reference_chain(D, recon, source, mi, P["bd"], P["last_levels"], P["base_qindex"], P["grain_set"])
        for k in ("dbk", "cdef"):
            assert pc.plane_digest(ref[k])[0] == want["digest_" + k][0], (name, k, "the reference's chain is not the chain fixture's")
        _, base = lu.picture_units(pc.W, pc.H)
        tables = tuple(want[k] for k in fu.INPUT_KEYS)
        opened[name] = (P, ref, source, base, tables)
        R = mg_lr.Reference(L, pc.W, pc.H, P["bd"], ref["cdef"], ref["dbk"], source)
        for s in grid:
            results[name, s] = reference_finish(L, fu.chain_rates(*s), base, *tables)
            check_restatement(results[name, s], fu.chain_rates(*s), base, tables, f"picture {name}, setting {s}")
        R.close()
    # choose the settings: the named ones, then whatever frame type is still missing
    chosen = {n: list(v) for n, v in NAMED_SETTINGS.items()}
    types_of = lambda sel: {int(t) for n, ss in sel.items() for s in ss for t in results[n, s]["frame_type"]}  # noqa: E731
    for t in range(4):
        if t in types_of(chosen):
            continue
        for (n, s), r in results.items():
            if t in r["frame_type"].tolist() and s not in chosen[n] and len(chosen[n]) < MAX_SETTINGS:
                chosen[n].append(s)
                break
    for n in chosen:                       # every picture runs an ordinary setting too
        if (60000, 800) not in chosen[n] and len(chosen[n]) < MAX_SETTINGS:
            chosen[n].append((60000, 800))
    for name, ss in chosen.items():
        P, ref, source, base, tables = opened[name]
        out[f"{name}_settings"] = np.array(ss, np.int64)
        R = mg_lr.Reference(L, pc.W, pc.H, P["bd"], ref["cdef"], ref["dbk"], source)
        for k, s in enumerate(ss):
            r = results[name, s]
            restored = mg_sgr.reference_filter(R, r["frame_type"], base, r["unit_type"], tables[1], tables[3])
            r["digest_restored"] = pc.plane_digest(restored)
            print("picture", name, "setting", s, "frame types", r["frame_type"].tolist(), "unit types", r["unit_type"].tolist())
        R.close()
        for key in fu.OUTPUT_KEYS + ("digest_restored",):
            out[f"{name}_{key}"] = np.stack([results[name, s][key] for s in ss])

    def chroma_all_three(n, s):
        r = results[n, s]
        return any(set(r["unit_type"][base[p]:base[p + 1]].tolist()) == {0, 1, 2} for p in (1, 2))
    base = opened["A"][3]
    facts = {"all four frame types occur": types_of(chosen) == {0, 1, 2, 3},
             "(B, 10^7, 2^22) has a chroma plane with all three unit types": chroma_all_three("B", (10_000_000, 1 << 22)),
             "(C, 2*10^6, 2^18) has a chroma plane with all three unit types": chroma_all_three("C", (2_000_000, 1 << 18)),
             "(A, 10^7, 2^22) has NONE planes": 0 in results["A", (10_000_000, 1 << 22)]["frame_type"].tolist(),
             "(A, 60000, 2^26) has self-guided planes": 2 in results["A", (60000, 1 << 26)]["frame_type"].tolist(),
             "at most four settings a picture": all(len(v) <= MAX_SETTINGS for v in chosen.values())}
    return facts


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "finish"))
        L = build_driver(os.path.join(tmp, "finish"))
        cases = fu.constructed_cases()
        out["names"] = np.array([c["name"] for c in cases])
        done = []
        for i, c in enumerate(cases):
            w, h, us = c["geom"]
            counts = open_geometry(L, w, h, us)
            assert counts == fu.unit_counts(w, h, us), (c["name"], counts)
            base = fu.unit_base_of(counts)
            tables = tuple(c[k] for k in fu.INPUT_KEYS)
            ref = reference_finish(L, c["rates"], base, *tables)
            L.drv_lr_close()
            check_restatement(ref, c["rates"], base, tables, c["name"])
            done.append(dict(c, unit_base=base, **ref))
            print(c["name"], "units", counts, "frame types", ref["frame_type"].tolist(), "n_tried", ref["n_tried"].tolist())
        missing = [k for k, v in fu.coverage(done).items() if not v]
        assert not missing, ("the constructed cases do not contain", missing)
        out["geom"] = np.array([[d["geom"][0], d["geom"][1], *d["geom"][2]] for d in done], np.int32)
        out["unit_base"], out["range"] = np.array([d["unit_base"] for d in done], np.int32), np.array([d["range"] for d in done], np.int32)
        out["rates"] = np.stack([fu.rates_array(d["rates"]) for d in done])
        for k in fu.INPUT_KEYS + ("unit_type", "best_rtype"):
            out[k] = np.concatenate([d[k] for d in done])
        for k in fu.RESULT_KEYS:
            out[k] = np.stack([d[k] for d in done])

        rng = np.random.default_rng(7)
        leaf = leaf_sample(rng)
        wb, sb = reference_bits(L, *leaf)
        for k, v in zip(("win", "taps", "ref", "sgr", "sgr_ref", "wiener_bits", "sgr_bits"), (*leaf, wb, sb)):
            out["leaf_" + k] = v.astype(np.int8)
        for j in range(len(wb)):
            assert fu.count_wiener_bits(int(leaf[0][j]), leaf[1][j].tolist(), leaf[2][j].tolist()) == wb[j]
            assert fu.count_sgrproj_bits(int(leaf[3][j][0]), leaf[3][j][1:].tolist(), leaf[4][j].tolist()) == sb[j]

        facts = chain_part(L, mg_chain.Drivers(tmp), out)
        missing = [k for k, v in facts.items() if not v]
        assert not missing, ("the chain settings do not give", missing)
    mg_cdef.save(fu.FIXTURE, out)
    mg_lr.print_sizes(out)
    print(f"wrote {fu.FIXTURE}: {os.path.getsize(fu.FIXTURE)} bytes")
    assert os.path.getsize(fu.FIXTURE) < SIZE_LIMIT


if __name__ == "__main__":
    main()
