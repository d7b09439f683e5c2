"""Writes tests/golden/ma_stats.npz from the reference's own motion-analysis functions (tests/golden/ref_ma_stats_driver.c, linked by the
recipe of oracle/ref_driver.py against the reference objects of the oracle build, oracle/_ref/obj_all).  Run in the build container only,
where the reference exists: the fixture is data.

    python tests/golden/make_golden_ma_stats.py

Cases (tests/ma_stats_util.py CASES): 64x64 (one SB), 136x72 (two complete SBs, four incomplete), 200x136 (ragged right and bottom), 256x256
(sixteen SBs, interior SBs with four neighbours).  Three groups of items per case, see zz_items, energy_items and table_items.  Contents:
  case [4][2]                      width, height
  c{c}_{group}_n                   items of a group, group one of zz, energy, tables
  c{c}_{group}{i}_{key}            inputs and what the reference left (ma_stats_util.ZZ_KEYS, ENERGY_KEYS, TABLE_KEYS); me is the raw bytes
                                   of [n_sb][85] svthip_me_cu_result
  tables: global_motion [6] is what MeBasedGlobalMotionDetection left; compare_global_motion is 0 for a table with an entry without a
  list-0 candidate, where the reference carries an earlier SB's vector and the entries promise nothing
  coverage_keys                    COVERAGE_KEYS, all reached: asserted here on the reference's results
The restatement (tests/ma_stats_util.py) is asserted equal to the reference on every output the reference has while generating."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import ma_stats_util as mu  # noqa: E402
import pa_stats_util as pu  # noqa: E402
from make_golden_cdef import save  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

ZZ_TARGETS = (0, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 6000)
COVERAGE_KEYS = tuple([f"zz_cost_{v}" for v in (0, 3, 10, 20, 30, 255)] + [f"non_moving_{v}" for v in (0, 10, 20, 30)] + [f"sad_{v}" for v in ZZ_TARGETS[1:9]]
                      + ["sad_0_off_grid_differs", "energy_flat_0", "energy_noise", "energy_checkerboard", "energy_64_is_not_the_sum", "energy_non_intra_sentinels",
                         "interval_low", "interval_compressed", "interval_clamped", "arm_inter", "arm_intra", "pan_1", "pan_0", "tilt_1", "tilt_0", "pan_12_of_16",
                         "pan_13_of_16", "negative_sum_with_remainder", "no_list0_entry"] + [f"pan_condition_{k}_alone" for k in "abcdef"]
                      + [f"flag{f}_{v}" for f in range(4) for v in (0, 1)] + ["deviation_15", "deviation_16", "deviation_20", "deviation_21", "ois_sad_0",
                                                                               "intensity_transition"])


def build_driver(out_dir):
    """ref_ma_stats_driver.c by the recipe of oracle/ref_driver.py, with its signatures"""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_ma_stats_driver.c"), out_dir)
    V = C.c_void_p
    L.drv_ma_open.argtypes = [C.c_int, C.c_int]
    L.drv_ma_zz.argtypes = [V] * 5
    L.drv_ma_energy.argtypes = [V, C.c_int, V, V, V]
    L.drv_ma_tables.argtypes = [V] * 9
    L.drv_ma_time.restype = C.c_double
    L.drv_ma_time.argtypes = [C.c_int, C.c_int]
    return L


def _ptr(a):
    return a.ctypes.data


def reference_zz(L, w, h, cur, prev):
    n = mu.n_sbs(w, h)
    assert L.drv_ma_open(w, h) == n
    cur, prev = np.ascontiguousarray(cur, np.uint8), np.ascontiguousarray(prev, np.uint8)
    sad, zz, nm = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    assert L.drv_ma_zz(_ptr(cur), _ptr(prev), _ptr(sad), _ptr(zz), _ptr(nm)) == 0
    return sad, zz, nm


def reference_energy(L, w, h, luma, intra, y_mean):
    n = mu.n_sbs(w, h)
    assert L.drv_ma_open(w, h) == n
    luma, y_mean = np.ascontiguousarray(luma, np.uint8), np.ascontiguousarray(y_mean, np.uint8)
    energy, mean = np.zeros((n, 5), np.uint64), np.zeros((n, 5), np.uint64)
    assert L.drv_ma_energy(_ptr(luma), int(intra), _ptr(y_mean), _ptr(energy), _ptr(mean)) == 0
    return energy, mean


def reference_tables(L, w, h, item):
    n = mu.n_sbs(w, h)
    assert L.drv_ma_open(w, h) == n
    keep = [np.ascontiguousarray(item[k]) for k in ("me", "cand", "y_mean", "variance", "ref_mean", "ref_var")]
    signals = np.ascontiguousarray(item["signals"], np.int32)
    gm, flags = np.zeros(6, np.int32), np.zeros((n, 4), np.uint8)
    assert L.drv_ma_tables(*[_ptr(a) for a in keep], _ptr(signals), _ptr(gm), _ptr(flags)) == 0
    return gm, flags


# ---------------------------------------------------------------------------------------------- inputs

def _base(w, h, k):
    y, x = np.mgrid[0:h, 0:w]
    return (64 + ((3 * x + 5 * y + 17 * k) & 127)).astype(np.uint8)      # 64..191: room for the deltas below on both sides


def zz_items(w, h):
    """[(cur, prev)]: the previous picture is the current one with, on the 4-grid of every complete SB, deltas of alternating sign that add up to that
    SB's target SAD (ZZ_TARGETS in turn, so that every case meets every ladder step from both sides), and with every sample OFF the 4-grid changed;
    a last pair differs only off the grid"""
    complete = [o for o in mu.sb_origins(w, h) if o[0] + 64 <= w and o[1] + 64 <= h]
    n_items = -(-len(ZZ_TARGETS) // len(complete))
    y, x = np.mgrid[0:h, 0:w]
    off_grid = ((x & 3) != 0) | ((y & 3) != 0)
    items = []
    for j in range(n_items + 1):
        cur = _base(w, h, j)
        prev = cur.copy()
        prev[off_grid] ^= 0x5a
        if j < n_items:
            for k, (sx, sy) in enumerate(complete):
                q, r = divmod(ZZ_TARGETS[(j * len(complete) + k) % len(ZZ_TARGETS)], 256)
                delta = np.full(256, q, np.int64)
                delta[:r] += 1
                delta[1::2] *= -1
                blk = prev[sy:sy + 64:4, sx:sx + 64:4]
                blk[:] = (blk.astype(np.int64) + delta.reshape(16, 16)).astype(np.uint8)
        items.append((cur, prev))
    return items


def energy_items(rng, w, h):
    """[(luma, slice_is_intra)]: flat 128, flat 255, noise, a full-swing checkerboard of single samples, one of 4x4 squares, a ramp with noise, and the
    noise picture again on a picture that is not intra"""
    y, x = np.mgrid[0:h, 0:w]
    noise = rng.integers(0, 256, (h, w)).astype(np.uint8)
    pics = [np.full((h, w), 128, np.uint8), np.full((h, w), 255, np.uint8), noise, (((x + y) & 1) * 255).astype(np.uint8),
            ((((x >> 2) + (y >> 2)) & 1) * 255).astype(np.uint8), np.clip(x + (y >> 1) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)]
    return [(p, 1) for p in pics] + [(noise, 0)]


def _word(distortion, mode=1):
    return np.uint32(int(distortion) | (1 << 20) | (mode << 24))


def _table_inputs(rng, w, h, item_index, mvs, no_l0=()):
    """ME rows, OIS words and the mean / variance tables of one item.  mvs: [n_sb] (x, y) of entry 0.  SB i takes distortion variant
    (i + item_index) % 8 and similarity variant (i + 2 * item_index) % 5, see make_golden_ma_stats.__doc__ and the assertions in main"""
    n = mu.n_sbs(w, h)
    me = np.zeros((n, 85), mu.ME_DTYPE)
    # random where the entries read (PUs 0..20) and next to it; the rest constant, to keep the fixture small
    for f in ("xMvL0", "yMvL0", "xMvL1", "yMvL1"):
        me[f][:, :21] = rng.integers(-60, 60, (n, 21))
    me["distortion"] = 77777
    me["distortion"][:, :21] = rng.integers(0, 4000, (n, 21, 3))
    me["direction"] = [0, 1, 2]
    me["totalMeCandidateIndex"] = 3
    cand = np.zeros((n, 85, 18), np.uint32)
    cand[:] = _word(123456, 9)
    cand[:, :6, :2] = (rng.integers(0, 16000, (n, 6, 2)).astype(np.uint32) | np.uint32(1 << 20) | (rng.integers(0, 35, (n, 6, 2)).astype(np.uint32) << np.uint32(24)))
    y_mean, variance = np.full((n, 85), 99, np.uint8), np.full((n, 85), 9999, np.uint16)
    y_mean[:, :2], variance[:, :2] = rng.integers(0, 256, (n, 2)), rng.integers(0, 16000, (n, 2))
    ref_mean, ref_var = np.zeros(n, np.uint8), np.zeros(n, np.uint16)
    for i in range(n):
        me["xMvL0"][i, 0], me["yMvL0"][i, 0] = mvs[i]
        if i % 3 == 1:      # the list-0 candidate second; and rows with one candidate
            me["direction"][i, 0] = [1, 0, 2]
        elif i % 3 == 2:
            me["totalMeCandidateIndex"][i, 0] = 1
        if i in no_l0:
            me["direction"][i, 0], me["totalMeCandidateIndex"][i, 0] = [1, 2, 0], 2
        v = (i + item_index) % 8
        if v < 5:           # 32x32 OIS SADs of 1000, ME SADs chosen for a deviation of exactly 15, 16, 20 (32x32) and 21 (64x64) percent; OIS SADs of 0
            for cu in range(1, 5):
                cand[i, cu, 0] = _word(0 if v == 4 else 1000, cu)
                me["distortion"][i, cu, 0] = 1000
            me["distortion"][i, 0, 0] = 4000
            if v < 3:
                me["distortion"][i, 1 + v, 0] = (1150, 1160, 1200)[v]
            elif v == 3:
                me["distortion"][i, 0, 0] = 4840
            else:
                me["distortion"][i, 0, 0] = 90000
        else:               # the three ranges of the interval index, for the ME sum and for the OIS sum
            lo, hi = ((0, 4000), (10000, 30000), (40000, 65000))[v - 5]
            me["distortion"][i, 5:21, 0] = rng.integers(lo, hi, 16)
            lo, hi = ((0, 16000), (40000, 120000), (150000, 261000))[v - 5]
            for cu in range(1, 5):
                cand[i, cu, 0] = _word(rng.integers(lo, hi), cu)
            me["distortion"][i, 0:5, 0] = rng.integers(0, 400000, 5)
        s = (i + 2 * item_index) % 5
        cm, cv = int(rng.integers(20, 230)), 1000
        rm, rv = ((cm, cv), (cm + 10, cv), (cm - 9, 1095), (cm, 1120), (cm, 0))[s]
        if s == 4:
            cv = 5
        y_mean[i, 0], variance[i, 0], ref_mean[i], ref_var[i] = cm, cv, rm, rv
    return {"me": me, "cand": cand, "y_mean": y_mean, "variance": variance, "ref_mean": ref_mean, "ref_var": ref_var}


def _signals(intra=0, tl=0, hl=3, used=0, transition=0):
    return np.array([intra, tl, hl, used, transition], np.int32)


PAN_PAIR = {"control": ((5, 1), (5, 1)), "a": ((5, 16), (5, 1)), "b": ((5, 1), (5, 16)), "c": ((-3, 1), (5, 1)), "d": ((1, 1), (5, 1)),
            "e": ((5, 1), (1, 1)), "f": ((21, 1), (5, 1))}


def pan_conditions(th, cur, cand):
    """the six conditions of CheckMvForPan, a..f in the order of the reference's &&"""
    return [cur[1] < 16, cand[1] < 16, cur[0] * cand[0] > 0, abs(cur[0]) >= th, abs(cand[0]) >= th, abs(cur[0] - cand[0]) < 16]


def table_items(rng, w, h):
    """[(name, inputs + signals + compare_global_motion)]"""
    n = mu.n_sbs(w, h)
    rnd = lambda lo, hi: [(int(a), int(b)) for a, b in rng.integers(lo, hi, (n, 2))]  # noqa: E731
    plans = [("pan", [(40 + i % 5, 3 - i % 2) for i in range(n)], _signals(used=1), ()),
             ("tilt", [(-2 + i % 3, -40 - (i * 7) % 11) for i in range(n)], _signals(), ()),
             ("pan_low_threshold", [(-5 - i % 4, 2) for i in range(n)], _signals(tl=3), ()),
             ("tilt_transition", [(3, 30 + i % 6) for i in range(n)], _signals(tl=1, hl=4, transition=1), ()),
             ("no_list0", [(40 + i % 5, 3) for i in range(n)], _signals(), (0,)),
             ("intra", rnd(-60, 60), _signals(intra=1), ()),
             ("random_high_threshold", rnd(-70, 70), _signals(hl=5, used=1), ()),
             ("random_low_threshold", rnd(-8, 8), _signals(tl=2, hl=2), ())]
    if (w, h) == (256, 256):
        rows = lambda k, extra=(): [(40 + i % 5, 3) if i < 4 * k or i in extra else (0, 0) for i in range(n)]  # noqa: E731
        plans += [("pan_12_of_16", rows(3), _signals(), ()), ("pan_13_of_16", rows(3, (12,)), _signals(), ())]
        for name, (cur, cnd) in PAN_PAIR.items():   # SBs 3, 13, 15 still; SB 12 looks at SB 8 alone: threshold 2
            mvs = [(0, 0) if i in (3, 13, 15) else cur if i == 12 else cnd if i == 8 else (5, 1) for i in range(n)]
            plans.append((f"pair_{name}", mvs, _signals(tl=3), ()))
    items = []
    for k, (name, mvs, signals, no_l0) in enumerate(plans):
        item = _table_inputs(rng, w, h, k, mvs, no_l0)
        item["signals"], item["compare_global_motion"] = signals, np.int32(not no_l0)
        items.append((name, item))
    return items


# ---------------------------------------------------------------------------------------------- main

def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    rng = np.random.default_rng(20261021)
    out = {"case": np.array(mu.CASES, np.int32)}
    cov = dict.fromkeys(COVERAGE_KEYS, False)
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for c, (w, h) in enumerate(mu.CASES):
            complete = mu.complete_sbs(w, h)
            # ---- ZZ SAD
            items = zz_items(w, h)
            out[f"c{c}_zz_n"] = np.int32(len(items))
            for i, (cur, prev) in enumerate(items):
                ref = reference_zz(L, w, h, cur, prev)
                mine = mu.zz_sad(cur, prev)
                for k, a, b in zip(mu.ZZ_KEYS[2:], mine, ref):
                    assert a.dtype == b.dtype and np.array_equal(a, b), ("the restatement differs from the reference", (w, h), i, k, a, b)
                    out[f"c{c}_zz{i}_{k}"] = b
                out[f"c{c}_zz{i}_cur"], out[f"c{c}_zz{i}_prev"] = cur, prev
                sad, zz, nm = ref
                for v in zz:
                    cov[f"zz_cost_{int(v)}"] = True
                for v in nm:
                    cov[f"non_moving_{int(v)}"] = True
                for v in sad[complete]:
                    if f"sad_{int(v)}" in cov:
                        cov[f"sad_{int(v)}"] = True
                if i == len(items) - 1:
                    assert not np.array_equal(cur, prev) and np.array_equal(cur[::4, ::4], prev[::4, ::4])
                    cov["sad_0_off_grid_differs"] |= bool((sad[complete] == 0).all())
                assert (sad[~complete] == 0xffffffff).all() and (zz[~complete] == 255).all()
            # ---- AC energy
            items = energy_items(rng, w, h)
            out[f"c{c}_energy_n"] = np.int32(len(items))
            for i, (luma, intra) in enumerate(items):
                y_mean = pu.block_stats(luma, luma[::2, ::2], luma[::2, ::2], 0)[0]
                ref = reference_energy(L, w, h, luma, intra, y_mean)
                mine = mu.ac_energy(luma, intra, y_mean)
                for k, a, b in zip(mu.ENERGY_KEYS[3:], mine, ref):
                    assert a.dtype == b.dtype and np.array_equal(a, b), ("the restatement differs from the reference", (w, h), i, k, a, b)
                    out[f"c{c}_energy{i}_{k}"] = b
                out[f"c{c}_energy{i}_luma"], out[f"c{c}_energy{i}_intra"], out[f"c{c}_energy{i}_y_mean"] = luma, np.int32(intra), y_mean
                e = ref[0]
                assert (e[~complete] == mu.SENTINEL).all() and (ref[1][~complete] == mu.SENTINEL).all()
                if intra:
                    cov["energy_flat_0"] |= i in (0, 1) and bool((e[complete] == 0).all())
                    cov["energy_noise"] |= i == 2 and bool((e[complete] > 0).all())
                    cov["energy_checkerboard"] |= i == 3 and bool((e[complete] > 0).all())
                    cov["energy_64_is_not_the_sum"] |= bool((e[complete, 0] != e[complete, 1:].sum(1)).any())
                else:
                    cov["energy_non_intra_sentinels"] |= bool((e == mu.SENTINEL).all() and (ref[1] == mu.SENTINEL).all())
            # ---- the table entries
            items = table_items(rng, w, h)
            out[f"c{c}_tables_n"] = np.int32(len(items))
            results = {}
            for i, (name, item) in enumerate(items):
                gm, flags = reference_tables(L, w, h, item)
                s = mu.signals_dict(item["signals"])
                mine = mu.all_tables(item, w, h)
                assert np.array_equal(mine["flags"], flags), ("the restatement differs from the reference", (w, h), name, "flags", mine["flags"], flags)
                if item["compare_global_motion"]:
                    assert np.array_equal(mine["global_motion"][:6], gm), ("the restatement differs from the reference", (w, h), name, mine["global_motion"], gm)
                    assert mine["global_motion"][11] == 0
                else:
                    cov["no_list0_entry"] |= mine["global_motion"][11] == 1
                item["global_motion"], item["flags"] = gm, flags
                for k in mu.TABLE_KEYS:
                    out[f"c{c}_tables{i}_{k}"] = item[k].view(np.uint8).reshape(-1) if k == "me" else item[k]
                results[name] = (gm, mine)
                # coverage, on the reference's results where it has them
                if s["slice_is_intra"]:
                    cov["arm_intra"] = True
                    assert not gm.any() and not flags.any()
                else:
                    cov["arm_inter"] = True
                    if item["compare_global_motion"]:
                        cov[f"pan_{int(gm[0])}"] = cov[f"tilt_{int(gm[1])}"] = True
                        counts = mine["global_motion"]
                        if gm[1] and counts[8] == counts[6]:     # every complete SB tilts: the sum is over all of them
                            total = int(item["me"][complete, 0]["yMvL0"].astype(np.int64).sum())
                            n = int(counts[8])
                            if total < 0 and total % n:
                                assert gm[5] == -(-total // n) and gm[5] != total // n     # towards zero, not towards minus infinity
                                cov["negative_sum_with_remainder"] = True
                    for f in range(4):
                        for v in (0, 1):
                            cov[f"flag{f}_{v}"] |= bool((flags[complete, f] == v).any())
                    cov["intensity_transition"] |= bool(s["intensity_transition_flag"])
                    for sb in np.flatnonzero(complete):
                        if flags[sb, 0]:
                            continue
                        ois = [mu.ois_sum32(item["cand"][sb])] + [int(mu.ois_distortion(item["cand"][sb, cu, 0])) for cu in range(1, 5)]
                        dev = [mu.sad_deviation(int(item["me"][sb][cu]["distortion"][0]), ois[cu]) for cu in range(5)]
                        quiet = not s["intensity_transition_flag"]
                        cov["ois_sad_0"] |= 0 in ois
                        if quiet and max(dev) == 15:
                            cov["deviation_15"] |= flags[sb, 2] == 0
                        if quiet and max(dev) == 16:
                            cov["deviation_16"] |= flags[sb, 2] == 1
                        if quiet and max(dev) == 20 and s["temporal_layer_index"] == 0:
                            cov["deviation_20"] |= flags[sb, 2] == 1 and flags[sb, 3] == 0
                        if quiet and max(dev) == 21 and s["temporal_layer_index"] == 0:
                            cov["deviation_21"] |= flags[sb, 2] == 1 and flags[sb, 3] == 1
                inter, intra_i = mine["inter_index"][complete], mine["intra_index"][complete]
                for idx in (intra_i,) if s["slice_is_intra"] else (inter, intra_i):
                    cov["interval_low"] |= bool(((idx > 0) & (idx <= 63)).any())
                    cov["interval_compressed"] |= bool(((idx > 63) & (idx < 127)).any())
                    cov["interval_clamped"] |= bool((idx == 127).any())
            if (w, h) == (256, 256):
                cov["pan_12_of_16"] = results["pan_12_of_16"][0][0] == 0 and results["pan_12_of_16"][1]["global_motion"][7] == 12
                cov["pan_13_of_16"] = results["pan_13_of_16"][0][0] == 1 and results["pan_13_of_16"][1]["global_motion"][7] == 13
                assert results["pair_control"][0][0] == 1 and all(pan_conditions(2, *PAN_PAIR["control"]))
                for k, name in enumerate("abcdef"):
                    held = pan_conditions(2, *PAN_PAIR[name])
                    assert [not v for v in held] == [j == k for j in range(6)], (name, held)
                    cov[f"pan_condition_{name}_alone"] = results[f"pair_{name}"][0][0] == 0
            print("case", c, (w, h), "zz", int(out[f"c{c}_zz_n"]), "energy", int(out[f"c{c}_energy_n"]), "tables", len(items))
    print("coverage", cov)
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    out["coverage_keys"] = np.array(COVERAGE_KEYS, dtype="U40")
    save(mu.FIXTURE, out)
    print(f"wrote {mu.FIXTURE}: {os.path.getsize(mu.FIXTURE) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
