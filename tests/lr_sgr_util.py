"""numpy / plain-integer restatement of the self-guided half of the reference's loop restoration (Source/Lib/Codec): the box filter
(EbRestoration.c:774-1064, the C forms), the projection (EbRestorationPick.c:485-599), the pixel projection error and its walk (:248-481), the
search of one unit over the 16 parameter sets (:602-670, :1670-1706) and the unit filter in filter geometry (EbRestoration.c:1066-1246).
Geometry and the stripe rule come from tests/lr_util.py.  Checked entry by entry against the reference's own run by
tests/test_lr_sgr_vs_ref.py; the device is checked against the same fixture by tests/test_lr_sgr_gpu.py."""
from fractions import Fraction

import numpy as np

import lr_util as lu
from abi_util import svtav1_hip

RST_BITS, PRJ_BITS, SGR_BITS, MTABLE_BITS, RECIP_BITS = 4, 7, 8, 20, 12
PRJ_MIN = (-96, -32)            # SGRPROJ_PRJ_MIN0, MIN1
PRJ_MAX = (31, 95)              # SGRPROJ_PRJ_MAX0, MAX1
N_PARAMS = 16
# sgr_params (EbRestoration.c:167-176): r[2], s[2]; r = 0 skips that filter
SGR_R = ((2, 1),) * 10 + ((0, 1),) * 4 + ((2, 0),) * 2
SGR_S = ((140, 3236), (112, 2158), (93, 1618), (80, 1438), (70, 1295), (58, 1177), (47, 1079), (37, 996), (30, 925), (25, 863),
         (-1, 2589), (-1, 1618), (-1, 1177), (-1, 925), (56, -1), (22, -1))
# x_by_xplus1 (EbRestoration.c:746-767): round(256 z / (z + 1)) with the two special ends 0 -> 1 and 255 -> 256
X_BY_XPLUS1 = np.array([1] + [(256 * z + (z + 1) // 2) // (z + 1) for z in range(1, 255)] + [256], np.int64)
ONE_BY_X = {9: 455, 25: 164}    # one_by_x[n - 1] = round(4096 / n)
U32 = 0xffffffff
DETAIL_DTYPE = svtav1_hip.SGRPROJ_DETAIL_DTYPE   # read from include/svtav1_hip.h by the package


def new_box_stats():
    return {k: 0 for k in ("r_both", "r1_only", "r0_only", "saturate_p", "z_ge_255")}


def new_filter_stats():
    return {k: 0 for k in ("above_only", "below_only", "both", "neither", "clip_lo", "clip_hi")}


def new_walk_stats():
    return {k: 0 for k in ("minus", "plus", "repeat", "skip_break", "tie", "range_stop_lo", "range_stop_hi")}


# ---------------------------------------------------------------- the box filter of one block
def _ab(D, h, w, bd, r, s, rows, st):
    """A and B of selfguided_restoration_[fast_]internal at rows `rows` (relative to the block) and columns -1 .. w"""
    n = (2 * r + 1) ** 2
    ri = np.asarray(rows) + 3
    S = np.zeros((len(ri), w + 2), np.int64)
    Q = np.zeros((len(ri), w + 2), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            blk = D[ri + dy][:, 2 + dx:2 + dx + w + 2]
            S += blk
            Q += blk * blk
    sh = bd - 8
    a = (Q + ((1 << (2 * sh)) >> 1)) >> (2 * sh)
    b = (S + ((1 << sh) >> 1)) >> sh
    sat = a * n < b * b
    p = np.where(sat, 0, a * n - b * b)
    z = (((p * s) & U32) + (1 << (MTABLE_BITS - 1)) & U32) >> MTABLE_BITS
    if st is not None:
        st["saturate_p"] += int(sat.sum())
        st["z_ge_255"] += int((z >= 255).sum())
    A = X_BY_XPLUS1[np.minimum(z, 255)]
    B = ((((256 - A) * S * ONE_BY_X[n]) & U32) + (1 << (RECIP_BITS - 1)) & U32) >> RECIP_BITS
    return A, B


def sgr_block(D, h, w, bd, ep, st=None):
    """av1_selfguided_restoration_c of an h x w block whose samples with their 3-sample border are D[(h + 6), (w + 6)]: flt0, flt1 (None
    for a radius of 0)"""
    D = D.astype(np.int64)
    dgd = D[3:3 + h, 3:3 + w]
    (r0, r1), (s0, s1) = SGR_R[ep], SGR_S[ep]
    if st is not None:
        st["r_both" if r0 and r1 else "r1_only" if r1 else "r0_only"] += 1
    flt0 = flt1 = None
    if r0:
        rows = np.arange(-1, h + 1, 2)
        A, B = _ab(D, h, w, bd, r0, s0, rows, st)
        flt0 = np.empty((h, w), np.int64)

        def comb(X, i):
            if i % 2 == 0:
                up, dn = X[i // 2], X[i // 2 + 1]
                return (up[1:w + 1] + dn[1:w + 1]) * 6 + (up[0:w] + dn[0:w] + up[2:w + 2] + dn[2:w + 2]) * 5
            m = X[(i + 1) // 2]
            return m[1:w + 1] * 6 + (m[0:w] + m[2:w + 2]) * 5
        for i in range(h):
            v = comb(A, i) * dgd[i] + comb(B, i)
            sft = SGR_BITS + (5 if i % 2 == 0 else 4) - RST_BITS
            flt0[i] = (v + (1 << (sft - 1))) >> sft
    if r1:
        A, B = _ab(D, h, w, bd, r1, s1, np.arange(-1, h + 1), st)
        def comb1(X):
            c = X[:, 1:w + 1]
            l, r = X[:, 0:w], X[:, 2:w + 2]
            return (c[1:h + 1] + l[1:h + 1] + r[1:h + 1] + c[0:h] + c[2:h + 2]) * 4 + (l[0:h] + l[2:h + 2] + r[0:h] + r[2:h + 2]) * 3
        v = comb1(A) * dgd + comb1(B)
        flt1 = (v + (1 << (SGR_BITS + 5 - RST_BITS - 1))) >> (SGR_BITS + 5 - RST_BITS)
    return flt0, flt1


def _pu(ss):
    return 64 >> ss


def sgr_unit_search_geometry(cdef, lim, bd, ep, ss, st=None):
    """apply_sgr: f0 = flt0 - u, f1 = flt1 - u of one unit (zeros for a radius of 0); processing units anchored at the unit's corner, the
    border read from the CDEF'd plane itself, clamped at the picture's edges"""
    h0, h1, v0, v1 = (int(v) for v in lim)
    ph, pw = cdef.shape
    f = [np.zeros((v1 - v0, h1 - h0), np.int64) for _ in range(2)]
    pu = _pu(ss)
    for y in range(v0, v1, pu):
        hh = min(pu, v1 - y)
        rows = np.clip(np.arange(y - 3, y + hh + 3), 0, ph - 1)
        for x in range(h0, h1, pu):
            ww = min(pu, h1 - x)
            cols = np.clip(np.arange(x - 3, x + ww + 3), 0, pw - 1)
            D = cdef[rows][:, cols]
            u = D[3:3 + hh, 3:3 + ww].astype(np.int64) << RST_BITS
            for k, flt in enumerate(sgr_block(D, hh, ww, bd, ep, st)):
                if flt is not None:
                    f[k][y - v0:y - v0 + hh, x - h0:x - h0 + ww] = flt - u
    return f


def plane_flt(cdef, limits, bd, ep, ss):
    """svthip_av1_[highbd_]selfguided_restoration_dev: flt0, flt1 (not minus u) of a whole plane in search geometry; None for radius 0"""
    out = [np.zeros(cdef.shape, np.int64) if SGR_R[ep][k] else None for k in range(2)]
    for lim in limits:
        h0, h1, v0, v1 = (int(v) for v in lim)
        f = sgr_unit_search_geometry(cdef, lim, bd, ep, ss)
        for k in range(2):
            if out[k] is not None:
                out[k][v0:v1, h0:h1] = f[k] + (cdef[v0:v1, h0:h1].astype(np.int64) << RST_BITS)
    return out


# ---------------------------------------------------------------- projection
def proj_sums(f0, f1, cdef_u, src_u):
    """the five sums of get_proj_subspace as integers: H00, H11, H01, C0, C1"""
    s = (src_u.astype(np.int64) << RST_BITS) - (cdef_u.astype(np.int64) << RST_BITS)
    return [int((f0 * f0).sum()), int((f1 * f1).sum()), int((f0 * f1).sum()), int((f0 * s).sum()), int((f1 * s).sum())]


def _rint(x):
    """rint in the default rounding mode: to nearest, ties to even"""
    return int(np.rint(np.float64(x)))


def solve(sums, size, ep):
    """the tail of get_proj_subspace_c in IEEE double with every product and difference rounded on its own (no fused multiply-add), then
    encode_xq: (xq[2], xqd[2])"""
    f = np.float64
    size = f(size)
    H00, H11, H01, C0, C1 = (f(int(v)) / size for v in sums)
    H10 = H01
    r0, r1 = SGR_R[ep]
    xq = [0, 0]
    if r0 == 0:
        if not H11 < 1e-8:
            xq[1] = _rint(C1 / H11 * f(128))
    elif r1 == 0:
        if not H00 < 1e-8:
            xq[0] = _rint(C0 / H00 * f(128))
    else:
        det = H00 * H11 - H01 * H10
        if not det < 1e-8:
            xq[0] = _rint((H11 * C0 - H01 * C1) / det * f(128))
            xq[1] = _rint((H00 * C1 - H10 * C0) / det * f(128))
    return xq, encode_xq(xq, ep)


def solve_fused(sums, size, ep, form=0):
    """what a compiler that contracts a * b - c * d would make of the two-filter arm: xq.  form 0: fma(a, b, -(c * d)), the second product
    rounded and the first exact; form 1: fma(-c, d, a * b), the first product rounded and the second exact.  Exact rational arithmetic with
    explicit roundings stands in for the fused instruction."""
    H00, H11, H01, C0, C1 = (Fraction(float(np.float64(int(v)) / np.float64(size))) for v in sums)
    rnd = lambda q: Fraction(_to_double(q))  # noqa: E731
    if form == 0:
        fms = lambda a, b, c, d: rnd(a * b - rnd(c * d))  # noqa: E731
    else:
        fms = lambda a, b, c, d: rnd(rnd(a * b) - c * d)  # noqa: E731
    det = fms(H00, H11, H01, H01)
    if det < Fraction(1e-8):
        return [0, 0]
    x0 = _to_double(fms(H11, C0, H01, C1)) / _to_double(det)
    x1 = _to_double(fms(H00, C1, H01, C0)) / _to_double(det)
    return [_rint(np.float64(x0) * 128), _rint(np.float64(x1) * 128)]


def fused_mask(sums, size, ep, xq):
    """bit f set: the fused form f of the two-filter arm gives another xq than the unfused evaluation"""
    if SGR_R[ep] != (2, 1):
        return 0
    return sum(1 << f for f in range(2) if solve_fused(sums, size, ep, f) != list(xq))


def _to_double(q):
    """the double nearest to the Fraction q (ties to even): Python's int / int division is correctly rounded"""
    return q.numerator / q.denominator


def clamp(v, lo, hi):
    return min(max(v, lo), hi)


def encode_xq(xq, ep):
    r0, r1 = SGR_R[ep]
    if r0 == 0:
        return [0, clamp(128 - xq[1], PRJ_MIN[1], PRJ_MAX[1])]
    x0 = clamp(xq[0], PRJ_MIN[0], PRJ_MAX[0])
    if r1 == 0:
        return [x0, clamp(128 - x0, PRJ_MIN[1], PRJ_MAX[1])]
    return [x0, clamp(128 - x0 - xq[1], PRJ_MIN[1], PRJ_MAX[1])]


def decode_xq(xqd, ep):
    r0, r1 = SGR_R[ep]
    if r0 == 0:
        return [0, 128 - xqd[1]]
    if r1 == 0:
        return [xqd[0], 0]
    return [xqd[0], 128 - xqd[0] - xqd[1]]


# ---------------------------------------------------------------- projection error and its walk
def proj_error(f0, f1, cdef_u, src_u, xqd, ep):
    """get_pixel_proj_error: the 8-bit and the 10-bit form are the same number, ((xq0 f0 + xq1 f1 + half) >> 11) + dat - src squared"""
    xq = decode_xq(xqd, ep)
    v = xq[0] * f0 + xq[1] * f1 + (1 << (RST_BITS + PRJ_BITS - 1))
    e = (v >> (RST_BITS + PRJ_BITS)) + cdef_u.astype(np.int64) - src_u.astype(np.int64)
    return int((e * e).sum())


def walk(err_fn, xqd, ep, st=None):
    """finer_search_pixel_proj_error with start_step 2: err_fn(xqd) -> error.  Returns the final error, xqd and the trace [(xqd, err)]."""
    xqd = [int(v) for v in xqd]
    trace = []

    def trial():
        e = err_fn(list(xqd))
        trace.append((list(xqd), e))
        return e

    err = trial()
    for s in (2, 1):
        for p in range(2):
            if SGR_R[ep][p] == 0:
                continue
            skip = False
            while True:
                if xqd[p] - s < PRJ_MIN[p]:
                    if st is not None:
                        st["range_stop_lo"] += 1
                    break
                xqd[p] -= s
                e2 = trial()
                if e2 > err:
                    xqd[p] += s
                    break
                if st is not None:
                    st["minus"] += 1
                    st["tie"] += e2 == err
                    st["repeat"] += skip
                err, skip = e2, True
                if s != 2:
                    break
            if skip:
                if st is not None and p == 0 and SGR_R[ep][1]:
                    st["skip_break"] += 1
                break
            moved = False
            while True:
                if xqd[p] + s > PRJ_MAX[p]:
                    if st is not None:
                        st["range_stop_hi"] += 1
                    break
                xqd[p] += s
                e2 = trial()
                if e2 > err:
                    xqd[p] -= s
                    break
                if st is not None:
                    st["plus"] += 1
                    st["tie"] += e2 == err
                    st["repeat"] += moved
                err, moved = e2, True
                if s != 2:
                    break
    return err, xqd, trace


def max_walk_trials():
    """The first trial; at step 2 a parameter makes at most 63 trials: a run of accepted moves spans at most MAX - MIN = 127, so at most 63
    moves, and a failing trial replaces one of them (a failed minus attempt means xqd >= MIN + 2, which leaves at most 62 plus moves and
    one failing); both parameters: 126; at step 1 at most a minus and a plus trial per parameter: 4."""
    return 1 + 2 * ((PRJ_MAX[0] - PRJ_MIN[0]) // 2) + 2 * 2


# ---------------------------------------------------------------- the search of one unit
def search_unit(cdef, src, lim, bd, ss, st_box=None, st_walk=None, keep_trace=True):
    """search_selfguided_restoration: the detail record per ep, the traces, and (ep, xqd) of the best (strict <, ep ascending)"""
    h0, h1, v0, v1 = (int(v) for v in lim)
    cu, su = cdef[v0:v1, h0:h1], src[v0:v1, h0:h1]
    size = (v1 - v0) * (h1 - h0)
    det = np.zeros(N_PARAMS, DETAIL_DTYPE)
    traces, best = [], None
    for ep in range(N_PARAMS):
        f0, f1 = sgr_unit_search_geometry(cdef, lim, bd, ep, ss, st_box)
        sums = proj_sums(f0, f1, cu, su)
        xq, xqd = solve(sums, size, ep)
        err, fin, trace = walk(lambda q: proj_error(f0, f1, cu, su, q, ep), xqd, ep, st_walk)
        det[ep] = (sums, xq, xqd, fin, err, len(trace), 0)
        traces.append(trace)
        if best is None or err < best[0]:
            best = (err, ep, fin)
    return det, traces, (best[1], best[2][0], best[2][1])


# ---------------------------------------------------------------- the unit filter, filter geometry
def filter_unit(cdef, dbk, lim, ep, xqd, bd, ss, st=None):
    """the restored samples of one RESTORE_SGRPROJ unit (sgrproj_filter_stripe[_highbd] per stripe, apply_selfguided_restoration_c per
    processing-unit-wide column block), the stripe rule as in lr_util.filter_unit"""
    h0, h1, v0, v1 = (int(v) for v in lim)
    ph, pw = cdef.shape
    out = np.empty((v1 - v0, h1 - h0), cdef.dtype)
    xq = decode_xq([int(v) for v in xqd], ep)
    top = (1 << bd) - 1
    for (y0, y1, above, below) in lu.stripes(v0, v1, ph, ss):
        if st is not None:
            st["both" if above and below else "above_only" if above else "below_only" if below else "neither"] += 1
        for x in range(h0, h1, _pu(ss)):
            ww = min(_pu(ss), h1 - x)
            cols = np.clip(np.arange(x - 3, x + ww + 3), 0, pw - 1)
            rows = []
            for r in range(y0 - 3, y1 + 3):
                if r < y0 and above:
                    rows.append(dbk[max(r, y0 - 2)][cols])
                elif r >= y1 and below:
                    rows.append(dbk[min(min(r, y1 + 1), ph - 1)][cols])
                else:
                    rows.append(cdef[min(max(r, 0), ph - 1)][cols])
            D = np.array(rows, np.int64)
            hh = y1 - y0
            u = D[3:3 + hh, 3:3 + ww] << RST_BITS
            v = u << PRJ_BITS
            for k, flt in enumerate(sgr_block(D, hh, ww, bd, ep)):
                if flt is not None:
                    v = v + xq[k] * (flt - u)
            w16 = (v + (1 << (PRJ_BITS + RST_BITS - 1))) >> (PRJ_BITS + RST_BITS)
            if st is not None:
                st["clip_lo"] += int((w16 < 0).sum())
                st["clip_hi"] += int((w16 > top).sum())
            out[y0 - v0:y1 - v0, x - h0:x - h0 + ww] = np.clip(w16, 0, top)
    return out


def trial_sse(cdef, dbk, src, lim, ep, xqd, bd, ss, st=None):
    h0, h1, v0, v1 = (int(v) for v in lim)
    d = filter_unit(cdef, dbk, lim, ep, xqd, bd, ss, st).astype(np.int64) - src[v0:v1, h0:h1].astype(np.int64)
    return int((d * d).sum())


def filter_frame(cdef, dbk, width, height, bd, frame_type, unit_type, unit_taps, unit_sgr, st=None):
    """av1_loop_restoration_filter_frame for the three unit types; unit_sgr[unit] = ep, xqd0, xqd1, 0"""
    planes, base = lu.picture_units(width, height)
    out = []
    for p in range(3):
        o = cdef[p].copy()
        if frame_type[p] != lu.RESTORE_NONE:
            for i, lim in enumerate(planes[p][0]):
                u = base[p] + i
                h0, h1, v0, v1 = (int(v) for v in lim)
                if unit_type[u] == lu.RESTORE_WIENER:
                    o[v0:v1, h0:h1] = lu.filter_unit(cdef[p], dbk[p], lim, unit_taps[u][:8], unit_taps[u][8:], bd, int(p > 0))
                elif unit_type[u] == lu.RESTORE_SGRPROJ:
                    o[v0:v1, h0:h1] = filter_unit(cdef[p], dbk[p], lim, int(unit_sgr[u][0]), unit_sgr[u][1:3], bd, int(p > 0), st)
        out.append(o)
    return out


# ---------------------------------------------------------------- the fixture
def load_case(z, lrz, c):
    """one case of tests/golden/lr_sgr.npz; the pictures of most cases are those of tests/golden/lr.npz (lrz)"""
    lc = int(z["lr_case"][c])
    if lc >= 0:
        F = lu.load_case(lrz, lc)
        out = {k: F[k] for k in ("w", "h", "bd", "src", "dbk", "cdef")}
    else:
        w, h, bd = (int(v) for v in z[f"x{c}_size"])
        dt = np.uint16 if bd > 8 else np.uint8
        src = [z[f"x{c}_src_{p}"] for p in range(3)]
        dbk = [(src[p].astype(np.int32) + z[f"x{c}_dbk_d{p}"]).astype(dt) for p in range(3)]
        cdef = [(dbk[p].astype(np.int32) + z[f"x{c}_cdef_d{p}"]).astype(dt) for p in range(3)]
        out = {"w": w, "h": h, "bd": bd, "src": src, "dbk": dbk, "cdef": cdef}
    planes, base = lu.picture_units(out["w"], out["h"])
    out["base"], out["limits"] = base, [pl[0] for pl in planes]
    out["plane"] = [0 if u < base[1] else 1 if u < base[2] else 2 for u in range(base[3])]
    out["unit_size"] = lu.unit_sizes(out["w"], out["h"])
    for k in ("detail", "sgrproj", "sse", "fsums", "ftype", "utype", "utaps", "usgr", "trace_xq", "trace_err"):
        out[k] = z[f"c{c}_{k}"]
    out["fdump"] = z.get(f"c{c}_fdump")
    dt = out["cdef"][0].dtype
    out["out"] = [[(out["cdef"][p].astype(np.int32) + z[f"c{c}_out{r}_d{p}"]).astype(dt) if out["ftype"][r][p] else None for p in range(3)]
                  for r in range(len(out["ftype"]))]
    return out


def case_traces(F, cap):
    """per (unit, ep) the recorded trials [(xq, err)], at most `cap` of each walk"""
    at, out = 0, {}
    for u in range(F["base"][3]):
        for ep in range(N_PARAMS):
            n = min(int(F["detail"][u][ep]["n_trials"]), cap)
            out[(u, ep)] = [([int(v) for v in F["trace_xq"][i]], int(F["trace_err"][i])) for i in range(at, at + n)]
            at += n
    return out
