"""The restoration decision (rest_finish_search, Codec/EbRestorationPick.c:1971-2040) restated for the tests: the four walks over the units
of a plane, the bit counts, the plane's choice.  TEST INFRASTRUCTURE: numpy and Python integers only, no reference code.

Inputs are the tables the two searches leave, in the device layouts: wiener_sse[units][2], taps[units][16], sgr_sse[units],
sgrproj[units][4], with unit_base[4] and the rates as a dict {rdmult, wiener_cost[2], sgrproj_cost[2], switchable_cost[3]}.
Costs are Python floats, which are IEEE doubles: RDCOST_DBL in the reference's order of operations.

Also here: the fixture tests/golden/lr_finish.npz (written by tests/golden/make_golden_lr_finish.py from the reference's own walk), the
constructed cases the generator feeds the reference, and what the issue's coverage list asks of them."""
import os

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "lr_finish.npz")
INT64_MAX = (1 << 63) - 1
NONE, WIENER, SGRPROJ, SWITCHABLE = 0, 1, 2, 3
TAP_MIN, TAP_MAX, TAP_K, TAP_MID = (-5, -23, -17), (10, 8, 46), (1, 2, 3), (3, -7, 15)
PRJ_MIN, PRJ_MAX, PRJ_K, PRJ_MID = (-96, -32), (31, 95), 4, (-32, 31)
SGR_SET_BITS, COST_SHIFT = 4, 9
RESULT_KEYS = ("sse", "bits", "cost", "frame_type", "n_tried")


# ---------------------------------------------------------------- bit counts (Codec/EbEntropyCoding.c:3375-3393, :3427-3432, :3488-3540)
def count_quniform(n, v):
    if n <= 1:
        return 0
    length = (n - 1).bit_length()
    return length - 1 if v < (1 << length) - n else length


def count_subexpfin(n, k, v):
    count, i, mk = 0, 0, 0
    while True:
        b = k + i - 1 if i else k
        a = 1 << b
        if n <= mk + 3 * a:
            return count + count_quniform(n - mk, v - mk)
        count += 1
        if v < mk + a:
            return count + b
        i, mk = i + 1, mk + a


def recenter_nonneg(r, v):
    return v if v > 2 * r else (v - r) * 2 if v >= r else (r - v) * 2 - 1


def count_refsubexpfin(n, k, ref, v):
    """aom_count_primitive_refsubexpfin on symbols ref, v in [0, n)"""
    return count_subexpfin(n, k, recenter_nonneg(ref, v) if 2 * ref <= n else recenter_nonneg(n - 1 - ref, n - 1 - v))


def coded_taps(taps16):
    """vfilter[0..2], hfilter[0..2] of a [16] taps row"""
    return [int(taps16[j]) for j in (0, 1, 2, 8, 9, 10)]


def count_wiener_bits(win, taps, ref):
    """count_wiener_bits (:1107-1143) on coded_taps lists: win 5 leaves tap 0 of both filters out"""
    return sum(count_refsubexpfin(TAP_MAX[j % 3] - TAP_MIN[j % 3] + 1, TAP_K[j % 3], ref[j] - TAP_MIN[j % 3], taps[j] - TAP_MIN[j % 3])
               for j in range(6) if win == 7 or j % 3)


def sgr_radius(ep, k):
    return (0 if 10 <= ep < 14 else 2) if k == 0 else (1 if ep < 14 else 0)


def count_sgrproj_bits(ep, xqd, ref):
    """count_sgrproj_bits (:673-688): the set, and an xqd only where the set's radius is not 0"""
    return SGR_SET_BITS + sum(count_refsubexpfin(PRJ_MAX[k] - PRJ_MIN[k] + 1, PRJ_K, ref[k] - PRJ_MIN[k], xqd[k] - PRJ_MIN[k])
                              for k in range(2) if sgr_radius(ep, k))


# ---------------------------------------------------------------- costs
def rdcost(rdmult, bits, sse):
    """RDCOST_DBL(rdmult, bits >> 4, sse) (EbRestoration.h:387-389): two exact products, one rounded addition"""
    return float(bits >> 4) * float(rdmult) / 512.0 + float(sse) * 128.0


def rdcost_exact(rdmult, bits, sse):
    """the same number times 512 in Python integers, without any rounding"""
    return (bits >> 4) * rdmult + sse * 128 * 512


# ---------------------------------------------------------------- the walks
def in_range(plane, wiener_sse, taps, sgrproj):
    """False where the device refuses a unit: a counted tap of a unit that is not rejected outside its range, a set above 15, an xqd outside"""
    if int(wiener_sse[1]) != INT64_MAX:
        t = coded_taps(taps)
        if any(not TAP_MIN[j % 3] <= t[j] <= TAP_MAX[j % 3] for j in range(6) if plane == 0 or j % 3):
            return False
    return 0 <= int(sgrproj[0]) <= 15 and all(PRJ_MIN[k] <= int(sgrproj[1 + k]) <= PRJ_MAX[k] for k in range(2))


def finish_plane(plane, rates, wiener_sse, taps, sgr_sse, sgrproj):
    """one plane's units -> (result dict, unit_type[n], best_rtype[n][4])"""
    n, win, rm = len(sgr_sse), 7 if plane == 0 else 5, int(rates["rdmult"])
    wc, sc, xc = ([int(v) for v in rates[k]] for k in ("wiener_cost", "sgrproj_cost", "switchable_cost"))
    sse = [(int(wiener_sse[u][0]), int(wiener_sse[u][1]), int(sgr_sse[u])) for u in range(n)]
    tap = [coded_taps(taps[u]) for u in range(n)]
    sgr = [[int(v) for v in sgrproj[u][:3]] for u in range(n)]
    best = np.zeros((n, 4), np.uint8)
    n_tried = 4 if n > 1 else 3
    R = {"sse": np.zeros(4, np.int64), "bits": np.zeros(4, np.int64), "cost": np.zeros(4, np.float64), "frame_type": 0, "n_tried": n_tried}
    if not all(in_range(plane, wiener_sse[u], taps[u], sgrproj[u]) for u in range(n)):
        R["n_tried"] = 0
        return R, np.zeros(n, np.uint8), best
    total = [[0, 0] for _ in range(4)]                # rsc->sse, rsc->bits of each walk

    for u in range(n):                                # search_norestore_finish
        total[NONE][0] += sse[u][0]

    ref = list(TAP_MID) * 2                           # search_wiener_finish
    for u in range(n):
        if sse[u][1] == INT64_MAX:
            total[WIENER][0] += sse[u][0]
            total[WIENER][1] += wc[0]
            continue
        bits = wc[1] + (count_wiener_bits(win, tap[u], ref) << COST_SHIFT)
        take = rdcost(rm, bits, sse[u][1]) < rdcost(rm, wc[0], sse[u][0])
        best[u, 0] = WIENER if take else NONE
        total[WIENER][0] += sse[u][1 if take else 0]
        total[WIENER][1] += bits if take else wc[0]
        if take:
            ref = tap[u]

    ref = list(PRJ_MID)                               # search_sgrproj_finish
    for u in range(n):
        bits = sc[1] + (count_sgrproj_bits(sgr[u][0], sgr[u][1:], ref) << COST_SHIFT)
        take = rdcost(rm, bits, sse[u][2]) < rdcost(rm, sc[0], sse[u][0])
        best[u, 1] = SGRPROJ if take else NONE
        total[SGRPROJ][0] += sse[u][2 if take else 0]
        total[SGRPROJ][1] += bits if take else sc[0]
        if take:
            ref = sgr[u][1:]

    if n_tried == 4:                                  # search_switchable
        wref, sref = list(TAP_MID) * 2, list(PRJ_MID)
        for u in range(n):
            b_type, b_bits, b_cost = NONE, xc[0], rdcost(rm, xc[0], sse[u][0])
            for r in (WIENER, SGRPROJ):
                if best[u, r - 1] == NONE:
                    continue
                count = count_wiener_bits(win, tap[u], wref) if r == WIENER else count_sgrproj_bits(sgr[u][0], sgr[u][1:], sref)
                bits = xc[r] + (count << COST_SHIFT)
                cost = rdcost(rm, bits, sse[u][r])
                if cost < b_cost:
                    b_type, b_bits, b_cost = r, bits, cost
            best[u, 2] = b_type
            total[SWITCHABLE][0] += sse[u][b_type]
            total[SWITCHABLE][1] += b_bits
            if b_type == WIENER:
                wref = tap[u]
            if b_type == SGRPROJ:
                sref = sgr[u][1:]

    for r in range(n_tried):
        R["sse"][r], R["bits"][r], R["cost"][r] = total[r][0], total[r][1], rdcost(rm, total[r][1], total[r][0])
        if r == 0 or R["cost"][r] < R["cost"][R["frame_type"]]:
            R["frame_type"] = r
    ft = R["frame_type"]
    return R, (best[:, ft - 1].copy() if ft else np.zeros(n, np.uint8)), best


def finish(rates, unit_base, wiener_sse, taps, sgr_sse, sgrproj, plane_start=0, plane_end=3):
    """rest_finish_search for planes [plane_start, plane_end): {unit_type[units], best_rtype[units][4], sse[3][4], bits[3][4], cost[3][4],
    frame_type[3], n_tried[3]}; what lies outside the plane range is 0"""
    n = int(unit_base[3])
    out = {"unit_type": np.zeros(n, np.uint8), "best_rtype": np.zeros((n, 4), np.uint8), "sse": np.zeros((3, 4), np.int64),
           "bits": np.zeros((3, 4), np.int64), "cost": np.zeros((3, 4), np.float64), "frame_type": np.zeros(3, np.int32), "n_tried": np.zeros(3, np.int32)}
    for p in range(plane_start, plane_end):
        a, b = int(unit_base[p]), int(unit_base[p + 1])
        R, ut, best = finish_plane(p, rates, wiener_sse[a:b], taps[a:b], sgr_sse[a:b], sgrproj[a:b])
        out["unit_type"][a:b], out["best_rtype"][a:b] = ut, best
        for k in RESULT_KEYS:
            out[k][p] = R[k]
    return out


def rates_of(rdmult, wiener, sgrproj, switchable):
    return {"rdmult": int(rdmult), "wiener_cost": [int(v) for v in wiener], "sgrproj_cost": [int(v) for v in sgrproj],
            "switchable_cost": [int(v) for v in switchable]}


def rates_array(rates):
    """the rates as 8 int32: rdmult, wiener_cost[2], sgrproj_cost[2], switchable_cost[3] (the layout of svthip_rest_finish_rates)"""
    return np.array([rates["rdmult"], *rates["wiener_cost"], *rates["sgrproj_cost"], *rates["switchable_cost"]], np.int32)


def rates_from_array(a):
    a = [int(v) for v in a]
    return rates_of(a[0], a[1:3], a[3:5], a[5:8])


def taps_row(v, h=None):
    """a [16] taps row from three coded taps per filter: entry 3 is -2 * (f0 + f1 + f2), 4..6 mirror"""
    row = np.zeros(16, np.int16)
    for o, f in ((0, v), (8, v if h is None else h)):
        row[o:o + 3], row[o + 3], row[o + 4:o + 7] = f, -2 * sum(f), f[::-1]
    return row


# ---------------------------------------------------------------- the constructed cases
# A case: name, (width, height, unit_size[3]) (the reference's unit walk yields the unit counts), the rates, the plane range, and the
# tables over all units of the picture.  Tables are built per plane from unit lists: (sse_none, sse_wiener | None = rejected, taps (v, h),
# sse_sgr, (ep, xqd0, xqd1)).
ORDINARY = rates_of(65536, (300, 800), (250, 900), (200, 800, 1300))


def units_in(size, unit):
    return max((size + (unit >> 1)) // unit, 1)


def unit_counts(w, h, unit_size):
    return [units_in(w >> (p > 0), unit_size[p]) * units_in(h >> (p > 0), unit_size[p]) for p in range(3)]


def unit_base_of(counts):
    return [0, counts[0], counts[0] + counts[1], sum(counts)]


def random_unit(rng, plane, scale=1 << 16, reject=0.15):
    """an ordinary unit: SSEs around `scale`, taps and xqd anywhere in their ranges"""
    none = int(rng.integers(scale // 2, scale * 2))
    tap = [tuple(int(rng.integers(TAP_MIN[j], TAP_MAX[j] + 1)) if (plane == 0 or j) else 0 for j in range(3)) for _ in range(2)]
    wi = None if rng.random() < reject else int(none - rng.integers(-scale // 8, scale // 2))
    sg = int(none - rng.integers(-scale // 8, scale // 2))
    return (none, wi, tap, sg, (int(rng.integers(0, 16)), int(rng.integers(PRJ_MIN[0], PRJ_MAX[0] + 1)), int(rng.integers(PRJ_MIN[1], PRJ_MAX[1] + 1))))


def tables_of(planes):
    """planes: three unit lists -> (wiener_sse, taps, sgr_sse, sgrproj)"""
    units = [u for p in planes for u in p]
    n = len(units)
    ws, tp, ss, sg = np.zeros((n, 2), np.int64), np.zeros((n, 16), np.int16), np.zeros(n, np.int64), np.zeros((n, 4), np.int32)
    for i, (none, wi, tap, s, g) in enumerate(units):
        ws[i] = (none, INT64_MAX if wi is None else wi)
        if wi is not None:                       # a rejected unit's WienerInfo is the zeroed RestUnitSearchInfo's
            tp[i] = taps_row(tap[0], tap[1])
        ss[i], sg[i, :3] = s, g
    return ws, tp, ss, sg


def _case(name, geom, rates, planes, plane_range=(0, 3)):
    counts = unit_counts(*geom)
    planes = [p(counts[i]) if callable(p) else p for i, p in enumerate(planes)]     # a callable: that many ordinary units
    assert [len(p) for p in planes] == counts, (name, [len(p) for p in planes], counts)
    ws, tp, ss, sg = tables_of(planes)
    return {"name": name, "geom": geom, "rates": rates, "range": plane_range, "wiener_sse": ws, "taps": tp, "sgr_sse": ss, "sgrproj": sg}


def constructed_cases():
    """the cases of the issue's list, in a fixed order; deterministic"""
    rng = np.random.default_rng(20)
    cases = []
    rand = lambda p, n, **k: [random_unit(rng, p, **k) for _ in range(n)]  # noqa: E731
    fill = lambda p: (lambda n: rand(p, n))  # noqa: E731
    D = ((3, -7, 15), (3, -7, 15))
    unit = lambda none, wi, sg, tap=D, g=(0, -32, 31): (none, wi, tap, sg, g)  # noqa: E731

    # one unit per plane (n_tried 3) and two units per plane
    cases.append(_case("one_unit", (64, 64, (64, 64, 64)), ORDINARY, [rand(0, 1, reject=0), rand(1, 1, reject=0), rand(2, 1, reject=0)]))
    cases.append(_case("two_units", (128, 64, (64, 64, 64)), ORDINARY, [rand(0, 2), rand(1, 1), rand(2, 1)]))
    cases.append(_case("two_units_chroma", (256, 128, (128, 64, 64)), ORDINARY, [rand(0, 2), rand(1, 2), rand(2, 2)]))

    # accepted, rejected, offered but loses, accepted: the last unit's bits count against the first's taps / xqd.  320 x 64 with unit 64:
    # five luma units; chroma 160 x 32: 2 units
    far = ((10, 8, 46), (-5, -23, -17))
    w_plane = [unit(100000, 60000, 100000, far), unit(100000, None, 100000), unit(100000, 99999, 100000, ((0, 0, 0), (9, 7, 40))),
               unit(100000, 50000, 100000, ((10, 8, 45), (-5, -22, -17))), unit(100000, 70000, 100000)]
    s_plane = [unit(100000, 100000, 60000, D, (3, -90, 90)), unit(100000, 100000, 100001, D, (11, 0, 0)), unit(100000, 100000, 99999, D, (14, 10, 10)),
               unit(100000, 100000, 50000, D, (12, -96, 88)), unit(100000, 100000, 70000, D, (15, -91, 95))]
    cases.append(_case("wiener_order", (320, 64, (64, 64, 64)), ORDINARY, [w_plane, fill(1), fill(2)]))
    cases.append(_case("sgrproj_order", (320, 64, (64, 64, 64)), ORDINARY, [s_plane, fill(1), fill(2)]))

    # exact ties with rdmult 65536: cost = ((bits >> 4) + sse) * 128, so two candidates tie where their sse differ by what their
    # bits >> 4 differ.  Default taps and default xqd throughout, so the counts do not depend on which unit was taken before.
    dflt = list(TAP_MID) * 2
    bw = ORDINARY["wiener_cost"][1] + (count_wiener_bits(7, dflt, dflt) << COST_SHIFT)
    bw5 = ORDINARY["wiener_cost"][1] + (count_wiener_bits(5, dflt, dflt) << COST_SHIFT)
    xw = ORDINARY["switchable_cost"][1] + (count_wiener_bits(7, dflt, dflt) << COST_SHIFT)
    xs = ORDINARY["switchable_cost"][2] + (count_sgrproj_bits(0, PRJ_MID, PRJ_MID) << COST_SHIFT)
    d_unit = (bw >> 4) - (ORDINARY["wiener_cost"][0] >> 4)
    tie_w = [unit(500000, 500000 - d_unit, 900000), unit(500000, 500000 - d_unit - 1, 900000)]      # stays NONE; one less: Wiener
    cases.append(_case("tie_unit_wiener_none", (128, 64, (64, 64, 64)), ORDINARY, [tie_w, fill(1), fill(2)]))
    d_sw = (xw >> 4) - (xs >> 4)                                   # sse_w + (xw >> 4) == sse_s + (xs >> 4)
    tie_sw = [unit(900000, 400000, 400000 + d_sw), unit(900000, 400000, 400000 + d_sw - 1)]         # takes Wiener; one less: self-guided
    cases.append(_case("tie_switchable_wiener_sgrproj", (128, 64, (64, 64, 64)), ORDINARY, [tie_sw, fill(1), fill(2)]))
    # two frame types in a plane of one unit: NONE has 0 bits, WIENER bw: the unit takes Wiener (it compares against bits_none = 300) and
    # the plane's two costs are equal, which takes NONE; in the first chroma plane one less, which takes WIENER
    tie_f = [unit(500000, 500000 - (bw >> 4), 900000)]
    cases.append(_case("tie_frame_types", (64, 64, (64, 64, 64)), ORDINARY, [tie_f, [unit(500000, 500000 - (bw5 >> 4) - 1, 900000)], rand(2, 1, reject=0)]))

    # rounding: SSEs of 2^38 to 2^40 and an odd rdmult.  The two rate terms differ by dR * rdmult / 512 with dR the difference of the
    # bits >> 4; with dR odd and rdmult = -j / dR modulo 2^16 that is a multiple of 128 minus j / 512, less than the last place of a sum
    # near 2^46 (2^-6).  The SSEs differ by that multiple, so the Wiener cost is the smaller by j / 512 as integers -- integer arithmetic
    # would take Wiener; the first (j, SSE) of a fixed search where the two are the same double, which stays NONE, is taken.
    rnd_rates = dict(ORDINARY, wiener_cost=[ORDINARY["wiener_cost"][0] + 16, ORDINARY["wiener_cost"][1]])
    d_r = (bw >> 4) - (rnd_rates["wiener_cost"][0] >> 4)
    assert d_r % 2 == 1
    found = None
    for j in (1, 3, 5, 7):
        rm = -j * pow(d_r, -1, 1 << 16) % (1 << 16)
        q = d_r * rm + j >> 16
        for e in (38, 39, 40):
            for off in range(64):
                none = (1 << e) + off
                if found is None and rdcost_exact(rm, bw, none - q) < rdcost_exact(rm, rnd_rates["wiener_cost"][0], none) and \
                        rdcost(rm, bw, none - q) == rdcost(rm, rnd_rates["wiener_cost"][0], none):
                    found = (rm, none, none - q)
    assert found, "no rounding case within the search"
    rm, none, wi = found
    odd = dict(rnd_rates, rdmult=rm)
    rnd = [unit(none, wi, none + 900), unit((1 << 40) + 3, (1 << 40) + 3 - d_unit, (1 << 40) + 5), unit(none + 1, wi + 1, none + 901)]
    cases.append(_case("rounding", (192, 64, (64, 64, 64)), odd, [rnd, rand(1, 2, scale=1 << 38), rand(2, 2, scale=1 << 38)]))

    # coefficient extremes: every tap at MINV then MAXV against the other end, xqd at both range ends
    lo, hi = (TAP_MIN, TAP_MIN), (TAP_MAX, TAP_MAX)
    ext = [unit(100000, 50000, 50000, lo, (0, PRJ_MIN[0], PRJ_MIN[1])), unit(100000, 50000, 50000, hi, (0, PRJ_MAX[0], PRJ_MAX[1])),
           unit(100000, 50000, 50000, lo, (0, PRJ_MIN[0], PRJ_MAX[1])), unit(100000, 50000, 50000, hi, (0, PRJ_MAX[0], PRJ_MIN[1]))]
    clo, chi = ((0,) + TAP_MIN[1:],) * 2, ((0,) + TAP_MAX[1:],) * 2
    cext = [unit(100000, 50000, 50000, clo, (5, PRJ_MIN[0], PRJ_MIN[1])), unit(100000, 50000, 50000, chi, (5, PRJ_MAX[0], PRJ_MAX[1]))]
    cases.append(_case("extremes", (256, 64, (64, 64, 64)), ORDINARY, [ext, cext, cext[::-1]]))

    # each frame type winning somewhere; a switchable plane with all three unit types
    cheap = rates_of(60000, (300, 800), (250, 900), (200, 800, 1300))
    mixed = [unit(100000, 40000, 99000), unit(100000, 99990, 40000), unit(100000, 99990, 99990), unit(100000, 30000, 90000)]
    all_w = [unit(100000, 40000, 90000)] * 2
    all_s = [unit(100000, 90000, 40000)] * 2
    cases.append(_case("frame_types", (256, 128, (128, 64, 64)), cheap, [[unit(100000, 99999, 99999)] * 2, all_w, all_s]))
    cases.append(_case("switchable_mixed", (256, 64, (64, 64, 64)), cheap, [mixed, fill(1), fill(2)]))

    # unit counts: more than 64, more than 256 (1280 x 960 with unit 64: 20 x 15 = 300 luma, 10 x 8 = 80 chroma), luma != chroma, a subset
    cases.append(_case("many_units", (1280, 960, (64, 64, 64)), ORDINARY, [rand(0, 300), rand(1, 80), rand(2, 80)]))
    cases.append(_case("subset", (256, 128, (128, 64, 64)), ORDINARY, [rand(0, 2), rand(1, 2), rand(2, 2)], (1, 2)))

    # seeded random cases of 1 to 9 units a plane
    geoms = {}
    for w in range(64, 64 * 10, 64):
        for h in (64, 128, 192):
            for us in ((64, 64, 64), (128, 64, 64), (256, 128, 128), (128, 128, 128)):     # both chroma planes alike, as in AV1
                c = unit_counts(w, h, us)
                if max(c) <= 9:
                    geoms.setdefault(tuple(c), (w, h, us))
    keys = sorted(geoms)
    for i in range(40):
        c = keys[int(rng.integers(0, len(keys)))]
        rates = rates_of(int(rng.choice([5000, 60000, 65536, 2_000_000, 10_000_001])), (int(rng.integers(0, 2000)), int(rng.integers(0, 1 << int(rng.integers(8, 20)))),),
                         (int(rng.integers(0, 2000)), int(rng.integers(0, 1 << int(rng.integers(8, 20))))),
                         (int(rng.integers(0, 2000)), int(rng.integers(0, 1 << int(rng.integers(8, 20)))), int(rng.integers(0, 1 << int(rng.integers(8, 20))))))
        scale = 1 << int(rng.integers(10, 30))
        cases.append(_case(f"random_{i:02d}", geoms[c], rates, [rand(p, c[p], scale=scale) for p in range(3)]))
    return cases


# the settings of the chain pictures: wiener (300, X), sgrproj (250, 900), switchable (200, X, 1300)
CHAIN_RDMULT = (5000, 60000, 2_000_000, 10_000_000)
CHAIN_X = (800, 1 << 14, 1 << 18, 1 << 22, 1 << 26)


def chain_rates(rdmult, x):
    return rates_of(rdmult, (300, x), (250, 900), (200, x, 1300))


# ---------------------------------------------------------------- the fixture
_FIXTURE = {}


def fixture():
    if not _FIXTURE:
        _FIXTURE.update(np.load(FIXTURE))
    return _FIXTURE


OUTPUT_KEYS = ("unit_type", "best_rtype", "sse", "bits", "cost", "frame_type", "n_tried")
INPUT_KEYS = ("wiener_sse", "taps", "sgr_sse", "sgrproj")


def fixture_case(i):
    """case i of the fixture: name, geom, unit_base, rates (dict), range, the input tables and the reference's outputs"""
    z = fixture()
    at = int(z["unit_base"][:i, 3].sum())
    units = slice(at, at + int(z["unit_base"][i, 3]))
    c = {k: z[k][units] for k in INPUT_KEYS + ("unit_type", "best_rtype")}
    c.update({k: z[k][i] for k in RESULT_KEYS})
    g = [int(v) for v in z["geom"][i]]
    c.update(name=str(z["names"][i]), geom=(g[0], g[1], tuple(g[2:5])), unit_base=[int(v) for v in z["unit_base"][i]],
             rates=rates_from_array(z["rates"][i]), range=tuple(int(v) for v in z["range"][i]))
    return c


def n_cases():
    return len(fixture()["names"])


def chain_settings(name):
    """[(rdmult, x)] of picture `name` in the fixture"""
    return [tuple(int(v) for v in s) for s in fixture()[f"{name}_settings"]]


def chain_case(name, k):
    """setting k of chain picture `name`: rates and the reference's outputs, with digest_restored of the reference's frame filter"""
    z = fixture()
    c = {key: z[f"{name}_{key}"][k] for key in OUTPUT_KEYS + ("digest_restored",)}
    c["rates"] = chain_rates(*chain_settings(name)[k])
    return c


def first_difference(got, want, plane_range=(0, 3), unit_base=None):
    """the first output, in OUTPUT_KEYS order, at which got differs from want within the plane range (cost by bit pattern), or None"""
    ps, pe = plane_range
    for k in OUTPUT_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k in ("unit_type", "best_rtype"):
            if unit_base is not None:
                g, w = g[unit_base[ps]:unit_base[pe]], w[unit_base[ps]:unit_base[pe]]
        else:
            g, w = g[ps:pe], w[ps:pe]
        if k == "cost":
            g, w = np.ascontiguousarray(g, np.float64).view(np.int64), np.ascontiguousarray(w, np.float64).view(np.int64)
        if g.shape != w.shape or not np.array_equal(g, w):
            at = np.argwhere(g != w)[:4].tolist() if g.shape == w.shape else "shape"
            return f"{k}: differs at {at}"
    return None


def coverage(cases):
    """the issue's list evaluated on cases with their (reference) outputs: {item: holds}.  A case is a fixture_case-like dict."""
    ok = {}
    planes = []          # (case, plane, slice)
    for c in cases:
        for p in range(*c["range"]):
            planes.append((c, p, slice(c["unit_base"][p], c["unit_base"][p + 1])))
    count = lambda c, s: s.stop - s.start  # noqa: E731
    ok["a plane of one unit with n_tried 3"] = any(count(c, s) == 1 and c["n_tried"][p] == 3 for c, p, s in planes)
    ok["a plane of two units"] = any(count(c, s) == 2 and c["n_tried"][p] == 4 for c, p, s in planes)

    def ordered(col, sse_of):
        # accepted, rejected / offered-and-lost ..., accepted, in this order within one plane of at least five units
        for c, p, s in planes:
            if count(c, s) < 5:
                continue
            b = c["best_rtype"][s, col]
            rej = c["wiener_sse"][s, 1] == INT64_MAX
            state = 0
            for u in range(len(b)):
                acc = b[u] != 0
                if state == 0 and acc:
                    state = 1
                elif state == 1 and col == 0 and rej[u]:
                    state = 2
                elif state == 1 and col == 1 and not acc:
                    state = 2
                elif state == 2 and not acc and not (col == 0 and rej[u]):
                    state = 3
                elif state == 3 and acc:
                    return True
        return False
    ok["Wiener: accepted, rejected, offered but loses, accepted"] = ordered(0, None)
    ok["self-guided: accepted, loses, loses, accepted"] = ordered(1, None)
    classes = set()
    for c, p, s in planes:
        for e in c["sgrproj"][s, 0]:
            classes.add(0 if e < 10 else 1 if e < 14 else 2)
    ok["self-guided sets of all three radius classes"] = classes == {0, 1, 2}
    by_name = {c["name"]: c for c in cases}

    def named(n):
        return by_name.get(n)
    c = named("tie_unit_wiener_none")
    ok["tie unit Wiener vs none stays NONE"] = c is not None and c["best_rtype"][0, 0] == 0 and c["best_rtype"][1, 0] == 1 and _tie(c, 0, "unit_w")
    c = named("tie_switchable_wiener_sgrproj")
    ok["tie switchable Wiener vs self-guided takes Wiener"] = c is not None and c["best_rtype"][0, 2] == 1 and c["best_rtype"][1, 2] == 2 and _tie(c, 0, "sw")
    c = named("tie_frame_types")
    ok["tie of two frame types takes the lower"] = (c is not None and c["frame_type"][0] == 0 and c["cost"][0][0] == c["cost"][0][1]
                                                    and c["frame_type"][1] == 1)
    c = named("rounding")
    ok["rounding: differ exactly, equal in double"] = c is not None and _rounding(c)
    c = named("extremes")
    ok["taps at MINV and MAXV against the other end, xqd at both ends"] = c is not None and _extremes(c)
    fts = {int(c["frame_type"][p]) for c, p, s in planes}
    ok["each of the four frame types wins in some plane"] = fts == {0, 1, 2, 3}
    ok["a switchable plane with all three unit types"] = any(c["frame_type"][p] == 3 and set(c["unit_type"][s].tolist()) == {0, 1, 2} for c, p, s in planes)
    ok["a plane with more than 64 units"] = any(64 < count(c, s) <= 256 for c, p, s in planes)
    ok["a plane with more than 256 units"] = any(count(c, s) > 256 for c, p, s in planes)
    ok["luma and chroma counts differ"] = any(c["unit_base"][1] != c["unit_base"][2] - c["unit_base"][1] for c in cases)
    ok["a plane-subset case"] = any(c["range"] == (1, 2) for c in cases)
    ok["about 40 random cases"] = sum(c["name"].startswith("random_") for c in cases) >= 40
    return ok


def _tie(c, u, kind):
    rm, r = c["rates"]["rdmult"], c["rates"]
    none, wi, sg = int(c["wiener_sse"][u, 0]), int(c["wiener_sse"][u, 1]), int(c["sgr_sse"][u])
    tap, ref = coded_taps(c["taps"][u]), list(TAP_MID) * 2
    if kind == "unit_w":
        b = r["wiener_cost"][1] + (count_wiener_bits(7, tap, ref) << COST_SHIFT)
        return rdcost_exact(rm, b, wi) == rdcost_exact(rm, r["wiener_cost"][0], none)
    bw = r["switchable_cost"][1] + (count_wiener_bits(7, tap, ref) << COST_SHIFT)
    bs = r["switchable_cost"][2] + (count_sgrproj_bits(int(c["sgrproj"][u, 0]), [int(v) for v in c["sgrproj"][u, 1:3]], list(PRJ_MID)) << COST_SHIFT)
    return rdcost_exact(rm, bw, wi) == rdcost_exact(rm, bs, sg)


def _rounding(c):
    """some unit of the case whose Wiener and none costs differ as integers and are the same double, with an odd rdmult and SSEs of 2^38 or more"""
    rm, r = c["rates"]["rdmult"], c["rates"]
    if rm % 2 == 0:
        return False
    ref = list(TAP_MID) * 2
    for u in range(len(c["sgr_sse"])):
        none, wi = int(c["wiener_sse"][u, 0]), int(c["wiener_sse"][u, 1])
        if wi == INT64_MAX or min(none, wi) < 1 << 38:
            continue
        b = r["wiener_cost"][1] + (count_wiener_bits(7 if u < c["unit_base"][1] else 5, coded_taps(c["taps"][u]), ref) << COST_SHIFT)
        if rdcost_exact(rm, b, wi) != rdcost_exact(rm, r["wiener_cost"][0], none) and rdcost(rm, b, wi) == rdcost(rm, r["wiener_cost"][0], none):
            return True
        # the reference taps move only when the unit is taken; these units use default taps throughout
    return False


def _extremes(c):
    t = [coded_taps(c["taps"][u]) for u in range(4)]
    lo, hi = list(TAP_MIN) * 2, list(TAP_MAX) * 2
    g = c["sgrproj"][:4, 1:3].tolist()
    return (t[0] == lo and t[1] == hi and t[2] == lo and t[3] == hi and bool((c["best_rtype"][:4, 0] == 1).all()) and bool((c["best_rtype"][:4, 1] == 2).all())
            and g == [[PRJ_MIN[0], PRJ_MIN[1]], [PRJ_MAX[0], PRJ_MAX[1]], [PRJ_MIN[0], PRJ_MAX[1]], [PRJ_MAX[0], PRJ_MIN[1]]])
