"""numpy / plain-integer restatement of the Wiener half of the reference's loop restoration (Source/Lib/Codec): unit geometry
(EbRestoration.c:198-237, :1343-1389), statistics (EbRestorationPick.c:743-836), solve (:845-1104), the unit filter (EbRestoration.c:346-554,
:1172-1246; convolve.c:64-222), the unit SSE and the refinement walk (EbRestorationPick.c:1257-1366).  Checked entry by entry against the
reference's own run by tests/test_lr_vs_ref.py; the device is checked against the same fixture by tests/test_lr_gpu.py."""
import numpy as np

WIN, HALF = 7, 3
FILT_STEP = 128                 # WIENER_FILT_STEP
TAP_SCALE = 1 << 16             # WIENER_TAP_SCALE_FACTOR
NUM_ITERS = 5                   # NUM_WIENER_ITERS
TAP_MID = (3, -7, 15)
TAP_BITS = (4, 5, 6)
TAP_MIN = tuple(m - (1 << b) // 2 for m, b in zip(TAP_MID, TAP_BITS))
TAP_MAX = tuple(m - 1 + (1 << b) // 2 for m, b in zip(TAP_MID, TAP_BITS))
INT64_MAX = (1 << 63) - 1
RESTORE_NONE, RESTORE_WIENER, RESTORE_SGRPROJ = 0, 1, 2
ROUND0, ROUND1, FILTER_BITS = 3, 11, 7


# ---------------------------------------------------------------- geometry
def unit_sizes(width, height):
    luma = 256 if width * height > 352 * 288 else 128
    return (luma, luma // 2, luma // 2)


def units_in(size, unit):
    return max((size + (unit >> 1)) // unit, 1)


def plane_units(pw, ph, unit, ss):
    """the units of one plane in raster order as rows (h_start, h_end, v_start, v_end), and the number of units per row"""
    off, ext = 8 >> ss, unit * 3 // 2
    out = []
    y0 = 0
    while y0 < ph:
        rem = ph - y0
        hh = rem if rem < ext else unit
        v0, v1 = max(0, y0 - off), y0 + hh
        if v1 < ph:
            v1 -= off
        x0 = 0
        while x0 < pw:
            rem = pw - x0
            ww = rem if rem < ext else unit
            out.append((x0, x0 + ww, v0, v1))
            x0 += ww
        y0 += hh
    return np.array(out, np.int32), units_in(pw, unit)


def picture_units(width, height, unit=None):
    """[(limits, units per row)] of the three planes and the index of each plane's first unit in the per-unit arrays"""
    unit = unit or unit_sizes(width, height)
    planes = [plane_units(width >> (p > 0), height >> (p > 0), unit[p], int(p > 0)) for p in range(3)]
    base = np.cumsum([0] + [len(pl[0]) for pl in planes])
    return planes, [int(b) for b in base]


def stripes(v0, v1, ph, ss):
    """the stripes of rows [v0, v1): (y0, y1, rows above substituted, rows below substituted)"""
    sh, off = 64 >> ss, 8 >> ss
    out = []
    y = v0
    while y < v1:
        k = (y + off) // sh
        nominal_end = (k + 1) * sh - off
        y1 = min(nominal_end, v1)
        out.append((y, y1, y != 0, nominal_end < ph))
        y = y1
    return out


# ---------------------------------------------------------------- statistics
def cdiv(a, b):
    """C division of integers: towards zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def compute_stats(dgd, src, lim, win, bd):
    """M[win^2], H[win^2][win^2], avg of one unit; the window reads the plane across unit edges and into a replicated border"""
    h0, h1, v0, v1 = (int(v) for v in lim)
    half = win >> 1
    P = np.pad(dgd.astype(np.int64), half, mode="edge")
    n = (v1 - v0) * (h1 - h0)
    avg = int(dgd[v0:v1, h0:h1].astype(np.int64).sum()) // n
    Y = np.empty((win * win, n), np.int64)
    for k in range(win):          # horizontal offset: the slow index
        for l in range(win):      # vertical offset
            Y[k * win + l] = P[v0 + l:v1 + l, h0 + k:h1 + k].reshape(-1) - avg
    X = src[v0:v1, h0:h1].astype(np.int64).reshape(-1) - avg
    M, H = Y @ X, Y @ Y.T
    if bd == 10:
        M, H = np.sign(M) * (np.abs(M) // 4), np.sign(H) * (np.abs(H) // 4)
    return M, H, avg


def unit_sse(a, b, lim):
    h0, h1, v0, v1 = (int(v) for v in lim)
    d = a[v0:v1, h0:h1].astype(np.int64) - b[v0:v1, h0:h1].astype(np.int64)
    return int((d * d).sum())


# ---------------------------------------------------------------- solve
def _i32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v & 0x80000000 else v


def _i16(v):
    v &= 0xffff
    return v - (1 << 16) if v & 0x8000 else v


def _wrap(i, win):
    return win - 1 - i if i >= (win >> 1) + 1 else i


def _linsolve(n, A, stride, b):
    x = [0] * n
    for k in range(n - 1):
        for i in range(n - 1, k, -1):
            if abs(A[(i - 1) * stride + k]) < abs(A[i * stride + k]):
                for j in range(n):
                    A[i * stride + j], A[(i - 1) * stride + j] = A[(i - 1) * stride + j], A[i * stride + j]
                b[i], b[i - 1] = b[i - 1], b[i]
        for i in range(k, n - 1):
            if A[k * stride + k] == 0:
                return None
            c, cd = A[(i + 1) * stride + k], A[k * stride + k]
            for j in range(n):
                A[(i + 1) * stride + j] -= cdiv(cdiv(c, 256) * A[k * stride + j], cd) * 256
            b[i + 1] -= cdiv(c * b[k], cd)
    for i in range(n - 1, -1, -1):
        if A[i * stride + i] == 0:
            return None
        c = 0
        for j in range(i + 1, n):
            c += cdiv(A[i * stride + j] * x[j], TAP_SCALE)
        x[i] = _i32(cdiv(TAP_SCALE * (b[i] - c), A[i * stride + i]))
    return x


def _update(win, M, H, a, b, which):
    """which 0: fix b, update a (update_a_sep_sym); 1: fix a, update b (update_b_sep_sym)"""
    win2, h1 = win * win, (win >> 1) + 1
    A, B = [0] * h1, [0] * (h1 * h1)
    for i in range(win):
        for j in range(win):
            if which == 0:
                A[_wrap(j, win)] += cdiv(M[i * win + j] * b[i], TAP_SCALE)
            else:
                A[_wrap(i, win)] += cdiv(M[i * win + j] * a[j], TAP_SCALE)
    for i in range(win):
        for j in range(win):
            for k in range(win):
                for l in range(win):
                    if which == 0:
                        hv = H[j * win * win2 + i * win + k * win2 + l]
                        B[_wrap(l, win) * h1 + _wrap(k, win)] += cdiv(cdiv(hv * b[i], TAP_SCALE) * b[j], TAP_SCALE)
                    else:
                        hv = H[i * win * win2 + j * win + k * win2 + l]
                        B[_wrap(j, win) * h1 + _wrap(i, win)] += cdiv(cdiv(hv * a[k], TAP_SCALE) * a[l], TAP_SCALE)
    e = h1 - 1
    for i in range(e):
        A[i] -= A[e] * 2 + B[i * h1 + e] - 2 * B[e * h1 + e]
    for i in range(e):
        for j in range(e):
            B[i * h1 + j] -= 2 * (B[i * h1 + e] + B[e * h1 + j] - 2 * B[e * h1 + e])
    S = _linsolve(e, B, h1, A)
    if S is None:
        return
    S = S + [TAP_SCALE] + [0] * (win - h1)
    for i in range(h1, win):
        S[i] = S[win - 1 - i]
        S[e] = _i32(S[e] - 2 * S[i])
    (a if which == 0 else b)[:] = S


def _finalize(win, f):
    half = win >> 1
    fi = [0] * 8
    for i in range(half):
        dividend = _i32(f[i] * FILT_STEP)
        fi[i] = _i16(cdiv(dividend - TAP_SCALE // 2, TAP_SCALE) if dividend < 0 else cdiv(dividend + TAP_SCALE // 2, TAP_SCALE))
    clip = lambda v, p: min(max(v, TAP_MIN[p]), TAP_MAX[p])  # noqa: E731
    if win == WIN:
        fi[0], fi[1], fi[2] = clip(fi[0], 0), clip(fi[1], 1), clip(fi[2], 2)
    else:
        fi[2] = clip(fi[1], 2)
        fi[1] = clip(fi[0], 1)
        fi[0] = 0
    fi[6], fi[5], fi[4] = fi[0], fi[1], fi[2]
    fi[3] = -2 * (fi[0] + fi[1] + fi[2])
    return fi


def _score(win, M, H, vf, hf):
    off, win2 = (WIN - win) >> 1, win * win
    a, b = [0] * WIN, [0] * WIN
    a[HALF] = b[HALF] = FILT_STEP
    for i in range(HALF):
        a[i] = a[WIN - 1 - i] = vf[i]
        b[i] = b[WIN - 1 - i] = hf[i]
        a[HALF] -= 2 * vf[i]
        b[HALF] -= 2 * hf[i]
    ab = [a[l + off] * b[k + off] for k in range(win) for l in range(win)]
    P = Q = 0
    for k in range(win2):
        P += cdiv(cdiv(ab[k] * M[k], FILT_STEP), FILT_STEP)
        for l in range(win2):
            q = ab[k] * H[k * win2 + l] * ab[l]
            for _ in range(4):
                q = cdiv(q, FILT_STEP)
            Q += q
    c = win2 >> 1
    return (Q - 2 * P) - (H[c * win2 + c] - 2 * M[c])


def solve(M, H, win):
    """start taps (vfilter[8], hfilter[8]) and whether compute_score rejects them"""
    M, H = [int(v) for v in np.asarray(M).reshape(-1)[:win * win]], [int(v) for v in np.asarray(H).reshape(-1)[:win ** 4]]
    off = (WIN - win) >> 1
    init = (3, -7, 15, FILT_STEP - 2 * (3 - 7 + 15), 15, -7, 3)
    a = [TAP_SCALE // FILT_STEP * init[i + off] for i in range(win)]
    b = list(a)
    for _ in range(1, NUM_ITERS):
        _update(win, M, H, a, b, 0)
        _update(win, M, H, a, b, 1)
    vf, hf = _finalize(win, a), _finalize(win, b)
    return vf, hf, _score(win, M, H, vf, hf) > 0


# ---------------------------------------------------------------- unit filter
def new_filter_stats():
    return {k: 0 for k in ("above_only", "below_only", "both", "neither", "clamp_lo", "clamp_hi", "clip_lo", "clip_hi")}


def filter_unit(cdef, dbk, lim, vf, hf, bd, ss, st=None):
    """the restored samples of one unit (wiener_filter_stripe[_highbd] per stripe, av1_[highbd_]wiener_convolve_add_src_c)"""
    h0, h1, v0, v1 = (int(v) for v in lim)
    ph, pw = cdef.shape
    cols = np.clip(np.arange(h0 - 3, h1 + 3), 0, pw - 1)
    out = np.empty((v1 - v0, h1 - h0), cdef.dtype)
    fh, fv = [int(v) for v in hf[:7]], [int(v) for v in vf[:7]]
    for (y0, y1, above, below) in stripes(v0, v1, ph, ss):
        rows = []
        for r in range(y0 - 3, y1 + 3):
            if r < y0 and above:
                rows.append(dbk[max(r, y0 - 2)][cols])
            elif r >= y1 and below:
                rows.append(dbk[min(min(r, y1 + 1), ph - 1)][cols])
            else:
                rows.append(cdef[min(max(r, 0), ph - 1)][cols])
        R = np.array(rows, np.int64)
        uw = h1 - h0
        s = (R[:, 3:3 + uw] << FILTER_BITS) + (1 << (bd + FILTER_BITS - 1))
        for k in range(7):
            s = s + R[:, k:k + uw] * fh[k]
        s = (s + (1 << (ROUND0 - 1))) >> ROUND0
        lim0 = (1 << (bd + 1 + FILTER_BITS - ROUND0)) - 1
        T = np.clip(s, 0, lim0)
        n = y1 - y0
        s2 = (T[3:3 + n] << FILTER_BITS) - (1 << (bd + ROUND1 - 1))
        for k in range(7):
            s2 = s2 + T[k:k + n] * fv[k]
        s2 = (s2 + (1 << (ROUND1 - 1))) >> ROUND1
        if st is not None:
            st["both" if above and below else "above_only" if above else "below_only" if below else "neither"] += 1
            st["clamp_lo"] += int((s < 0).sum())
            st["clamp_hi"] += int((s > lim0).sum())
            st["clip_lo"] += int((s2 < 0).sum())
            st["clip_hi"] += int((s2 > (1 << bd) - 1).sum())
        out[y0 - v0:y1 - v0] = np.clip(s2, 0, (1 << bd) - 1)
    return out


def trial_sse(cdef, dbk, src, lim, vf, hf, bd, ss, st=None):
    h0, h1, v0, v1 = (int(v) for v in lim)
    d = filter_unit(cdef, dbk, lim, vf, hf, bd, ss, st).astype(np.int64) - src[v0:v1, h0:h1].astype(np.int64)
    return int((d * d).sum())


def filter_frame(cdef, dbk, width, height, bd, frame_type, unit_type, unit_taps, unit=None, st=None):
    """av1_loop_restoration_filter_frame: the three planes; a plane whose frame type is RESTORE_NONE is returned as it is"""
    planes, base = picture_units(width, height, unit)
    out = []
    for p in range(3):
        o = cdef[p].copy()
        if frame_type[p] != RESTORE_NONE:
            for i, lim in enumerate(planes[p][0]):
                u = base[p] + i
                assert unit_type[u] in (RESTORE_NONE, RESTORE_WIENER)
                if unit_type[u] == RESTORE_WIENER:
                    h0, h1, v0, v1 = (int(v) for v in lim)
                    o[v0:v1, h0:h1] = filter_unit(cdef[p], dbk[p], lim, unit_taps[u][:8], unit_taps[u][8:], bd, int(p > 0), st)
        out.append(o)
    return out


# ---------------------------------------------------------------- the refinement walk
def new_walk_stats():
    return {k: 0 for k in ("minus", "plus", "repeat", "skip_break", "tie", "range_stop")}


def _move(f, p, d):
    f[p] += d
    f[WIN - 1 - p] += d
    f[HALF] -= 2 * d


def walk(err_fn, vf, hf, win, st=None):
    """finer_tile_search_wiener_seg as it is written: err_fn(vfilter, hfilter) -> SSE.  Returns the final error, the taps and the trace
    [(vfilter + hfilter, SSE)] of every trial in order."""
    off = (WIN - win) >> 1
    vf, hf = list(vf), list(hf)
    trace = []

    def trial():
        e = err_fn(vf, hf)
        trace.append((list(vf) + list(hf), e))
        return e

    err = trial()
    s = 4
    while s >= 1:
        for f in (hf, vf):
            for p in range(off, HALF):
                skip = False
                while True:
                    if f[p] - s >= TAP_MIN[p]:
                        _move(f, p, -s)
                        e2 = trial()
                        if e2 > err:
                            _move(f, p, s)
                        else:
                            if st is not None:
                                st["minus"] += 1
                                st["tie"] += e2 == err
                                st["repeat"] += skip and s == 4
                            err, skip = e2, True
                            if s == 4:
                                continue
                    elif st is not None:
                        st["range_stop"] += 1
                    break
                if skip:
                    if st is not None and p < HALF - 1:
                        st["skip_break"] += 1
                    break
                moved = False
                while True:
                    if f[p] + s <= TAP_MAX[p]:
                        _move(f, p, s)
                        e2 = trial()
                        if e2 > err:
                            _move(f, p, -s)
                        else:
                            if st is not None:
                                st["plus"] += 1
                                st["tie"] += e2 == err
                                st["repeat"] += moved and s == 4
                            err, moved = e2, True
                            if s == 4:
                                continue
                    elif st is not None:
                        st["range_stop"] += 1
                    break
        s >>= 1
    return err, vf, hf, trace


def max_walk_trials(win=WIN):
    """An upper bound of the number of trials of one walk, from its structure: the first trial; at step 4, per filter and tap, one minus
    attempt that fails and then at most (max - min) / 4 plus moves (or that many minus moves: fewer trials); at steps 2 and 1 at most
    one minus and one plus attempt per filter and tap."""
    off = (WIN - win) >> 1
    at4 = sum(1 + (TAP_MAX[p] - TAP_MIN[p]) // 4 for p in range(off, HALF))
    return 1 + 2 * at4 + 2 * 2 * 2 * (HALF - off)


# walk_step: the walk as a state machine, one call per trial.  State: taps, err, (s, filt, p, dir, skip), done, trials.
def walk_init(vf, hf, win, rejected=False):
    return {"v": list(vf), "h": list(hf), "err": INT64_MAX if rejected else 0, "s": 4, "filt": 0, "p": (WIN - win) >> 1, "dir": 0, "skip": 0,
            "phase": 0, "done": bool(rejected), "trials": 0, "off": (WIN - win) >> 1}


def _advance(S):
    """from the position (s, filt, p, dir) find the next trial: apply its move and return, or mark the walk done"""
    while not S["done"]:
        f, p, s = (S["h"], S["v"])[S["filt"]], S["p"], S["s"]
        if S["dir"] == 0:
            if f[p] - s >= TAP_MIN[p]:
                _move(f, p, -s)
                return
            if not S["skip"]:
                S["dir"] = 1
                continue
        elif f[p] + s <= TAP_MAX[p]:
            _move(f, p, s)
            return
        _next_tap(S)


def walk_step(S, sse):
    """consume the SSE of the trial of S's taps; leave the next candidate in S["v"], S["h"] or set S["done"] (taps = the best then)"""
    if S["done"]:
        return
    S["trials"] += 1
    if S["phase"] == 0:
        S["phase"], S["err"] = 1, sse
        _advance(S)
        return
    f, p, s = (S["h"], S["v"])[S["filt"]], S["p"], S["s"]
    d = -s if S["dir"] == 0 else s
    if sse > S["err"]:
        _move(f, p, -d)
        if S["dir"] == 0 and not S["skip"]:
            S["dir"] = 1
        else:
            _next_tap(S)
    else:
        S["err"] = sse
        if S["dir"] == 0:
            S["skip"] = 1
        if s != 4:
            _next_tap(S)
    _advance(S)


def _next_tap(S):
    """after the attempts on tap p end: the next tap, or past the last one when a minus move was accepted (`if (skip) break;`)"""
    p = HALF if S["skip"] else S["p"] + 1
    S["dir"], S["skip"] = 0, 0
    if p < HALF:
        S["p"] = p
        return
    S["p"] = S["off"]
    if S["filt"] == 0:
        S["filt"] = 1
        return
    S["filt"] = 0
    S["s"] >>= 1
    if S["s"] == 0:
        S["done"] = True


def walk_by_steps(err_fn, vf, hf, win):
    S = walk_init(vf, hf, win)
    trace = []
    while not S["done"]:
        e = err_fn(S["v"], S["h"])
        trace.append((list(S["v"]) + list(S["h"]), e))
        walk_step(S, e)
    return S["err"], S["v"], S["h"], trace


# ---------------------------------------------------------------- the fixture
def pack_upper(H, win):
    n = win * win
    return np.asarray(H).reshape(-1)[:n * n].reshape(n, n)[np.triu_indices(n)]


def load_case(z, c):
    """one case of tests/golden/lr.npz with its planes added up and H expanded"""
    w, h, bd = (int(v) for v in z["case"][c])
    dt = np.uint16 if bd > 8 else np.uint8
    src = [z[f"c{c}_src_{p}"] for p in range(3)]
    dbk = [(src[p].astype(np.int32) + z[f"c{c}_dbk_d{p}"]).astype(dt) for p in range(3)]
    cdef = [(dbk[p].astype(np.int32) + z[f"c{c}_cdef_d{p}"]).astype(dt) for p in range(3)]
    base = [int(v) for v in z[f"c{c}_base"]]
    H = np.zeros((base[3], 49 * 49), np.int64)
    hu, at = z[f"c{c}_Hu"], 0
    for u in range(base[3]):
        n = 49 if u < base[1] else 25
        m = np.zeros((n, n), np.int64)
        iu = np.triu_indices(n)
        m[iu] = hu[at:at + len(iu[0])]
        at += len(iu[0])
        H[u, :n * n] = (m + np.triu(m, 1).T).reshape(-1)
    out = {"w": w, "h": h, "bd": bd, "src": src, "dbk": dbk, "cdef": cdef, "base": base, "H": H, "win": [7 if u < base[1] else 5 for u in range(base[3])],
           "plane": [0 if u < base[1] else 1 if u < base[2] else 2 for u in range(base[3])]}
    for k in ("M", "avg", "start", "rejected", "sse", "final", "n_trials", "trace_taps", "trace_sse", "limits", "unit_size", "ftype", "utype", "utaps"):
        out[k] = z[f"c{c}_{k}"]
    out["out"] = [[(cdef[p].astype(np.int32) + z[f"c{c}_out{r}_d{p}"]).astype(dt) if out["ftype"][r][p] else None for p in range(3)]
                  for r in range(len(out["ftype"]))]
    return out
