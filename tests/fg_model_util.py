"""Film-grain estimation restated in numpy (TEST INFRASTRUCTURE): aom_noise_model_update (Codec/noise_model.c:1030-1147) and the sample work
of aom_flat_block_finder_run (:580-686), sequential over samples and vectorised over matrix entries, which keeps every rounding of the
reference: an elementwise numpy operation on float64 is the IEEE operation, and no sum here is left to np.sum / np.dot (they add pairwise).
Also the pictures, flat-block maps and cases of tests/golden/fg_model.npz, and the host's finish of the flat-block finder (score, sort,
union, :666-698) with math.exp, which is the libm exp the reference calls.

A state is a 0-d array of the header's svthip_film_grain_noise_state, features an array of svthip_film_grain_flat_block_features."""
import math
import os

import numpy as np

from svtav1_hip import _abi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "fg_model.npz")
STATE = _abi.dtype("svthip_film_grain_noise_state")
FEATURES = _abi.dtype("svthip_film_grain_flat_block_features")
BLOCK, LAG, COORDS, BINS = 32, 3, 24, 20
SHAPE_SQUARE = _abi.define("SVTHIP_FILM_GRAIN_NOISE_SHAPE_SQUARE")
OK, INSUFFICIENT, INTERNAL = (_abi.define("SVTHIP_FILM_GRAIN_NOISE_" + k) for k in ("OK", "INSUFFICIENT_FLAT_BLOCKS", "INTERNAL_ERROR"))
TABLES_DOUBLES = _abi.define("SVTHIP_FILM_GRAIN_FLAT_TABLES_DOUBLES")
TINY = 1.0e-16
CX = np.array([x for y in range(-LAG, 1) for x in range(-LAG, (0 if y == 0 else LAG + 1))])
CY = np.array([y for y in range(-LAG, 1) for x in range(-LAG, (0 if y == 0 else LAG + 1))])
assert len(CX) == COORDS
COVERAGE_KEYS = ("y_start_0", "y_start_lag", "x_start_0", "x_start_lag", "x_end_width", "x_end_flat_right", "x_end_not_flat_right", "x_end_is_1",
                 "gate_skips_block", "gate_keeps_narrow_column", "row_exchange", "status_ok", "status_insufficient", "status_internal", "chroma_fallback")

# (width, height, bit depth) of the fixture's pictures and, per picture, the cases: (flat map, planes variant)
PICTURES = ((64, 64, 8), (100, 72, 8), (96, 40, 10))
CASES = ((0, "all", "noisy"), (0, "checker", "noisy"), (0, "one", "noisy"), (0, "all", "luma_equal"), (0, "all", "chroma_equal"),
         (1, "all", "noisy"), (1, "checker", "noisy"), (1, "row", "noisy"), (1, "mixed", "noisy"),
         (2, "all", "noisy"), (2, "mixed", "noisy"), (2, "row", "noisy"), (2, "checker", "chroma_equal"))


def blocks_of(w, h):
    return (w + BLOCK - 1) // BLOCK, (h + BLOCK - 1) // BLOCK


def planes_of(p, variant="noisy"):
    """(data, denoised) of picture p: a smooth ramp plus seeded noise whose strength grows to the right, and a 3x3 box blur of it;
    luma_equal / chroma_equal make the denoised luma / chroma planes copies of the data"""
    w, h, bd = PICTURES[p]
    return make_planes(w, h, bd, np.random.default_rng([11, p]), variant)


def make_planes(w, h, bd, rng, variant="noisy"):
    """planes_of for any size (the probe's pictures)"""
    top, scale, dt = (1 << bd) - 1, 1 << (bd - 8), np.uint16 if bd > 8 else np.uint8
    data, den = [], []
    for k in range(3):
        pw, ph = w >> (k > 0), h >> (k > 0)
        yy, xx = np.mgrid[0:ph, 0:pw]
        ramp = 40 + 100 * xx / pw + 60 * yy / ph + 20 * k
        sigma = 1.2 + 2.8 * xx / pw + 0.9 * yy / ph
        d = np.clip(np.rint((ramp + sigma * rng.standard_normal((ph, pw))) * scale), 0, top).astype(np.int64)
        e = np.pad(d, 1, mode="edge")
        blur = sum(e[1 + dy:1 + dy + ph, 1 + dx:1 + dx + pw] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
        data.append(d.astype(dt))
        den.append(((blur + 4) // 9).astype(dt))
    if variant == "luma_equal":
        den[0] = data[0].copy()
    elif variant == "chroma_equal":
        den[1], den[2] = data[1].copy(), data[2].copy()
    else:
        assert variant == "noisy"
    return data, den


def flat_map(p, kind):
    w, h, _ = PICTURES[p]
    nbw, nbh = blocks_of(w, h)
    by, bx = np.mgrid[0:nbh, 0:nbw]
    if kind == "all":
        m = np.full((nbh, nbw), 255)
    elif kind == "checker":
        m = ((bx + by) % 2 == 0) * 255
    elif kind == "row":
        m = (by == nbh - 1) * 255
    elif kind == "mixed":
        m = np.where((bx * 3 + by) % 4 == 3, 0, np.where((bx + by) % 2, 1, 255))
    else:
        assert kind == "one"
        m = (bx + by == 0) * 255
    return np.ascontiguousarray(m, dtype=np.uint8)


def fixture():
    return np.load(FIXTURE)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def differing_fields(a, b):
    """names of the fields of two states whose bits differ (for a failure's message)"""
    out = []
    for which in ("latest", "combined"):
        for c in range(3):
            for k in a[which].dtype.names:
                if a[which][c][k].tobytes() != b[which][c][k].tobytes():
                    out.append(f"{which}[{c}].{k}")
    return out + [k for k in ("status",) if a[k] != b[k]]


# ---------------------------------------------------------------- linsolve and the equation systems

def linsolve(n, A, b, x, cov=None):
    """Codec/mathutils.h:26-60 on copies A (n x n) and b; x is written in place and keeps what it held behind a failure"""
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            for i in range(n - 1, k, -1):
                if abs(A[i - 1, k]) < abs(A[i, k]):
                    A[[i - 1, i]] = A[[i, i - 1]]
                    b[[i - 1, i]] = b[[i, i - 1]]
                    if cov is not None:
                        cov["row_exchange"] = True
            for i in range(k, n - 1):
                if abs(A[k, k]) < TINY:
                    return 0
                c = A[i + 1, k] / A[k, k]
                A[i + 1] -= c * A[k]
                b[i + 1] -= c * b[k]
        for i in range(n - 1, -1, -1):
            if abs(A[i, i]) < TINY:
                return 0
            c = np.float64(0)
            for j in range(i + 1, n):
                c += A[i, j] * x[j]
            x[i] = (b[i] - c) / A[i, i]
    return 1


class Channel:
    """aom_noise_state_t as aom_noise_model_init leaves it"""

    def __init__(self, n):
        self.n = n
        self.A, self.b, self.x = np.zeros((n, n)), np.zeros(n), np.zeros(n)
        self.ar_gain, self.num_observations = np.float64(1.0), 0
        self.sA, self.sb, self.sx = np.zeros((BINS, BINS)), np.zeros(BINS), np.zeros(BINS)
        self.total, self.num_equations = np.float64(0), 0

    def pack(self, out):
        n = self.n
        out["A"][:n * n], out["b"][:n], out["x"][:n] = self.A.ravel(), self.b, self.x
        out["ar_gain"], out["num_observations"] = self.ar_gain, self.num_observations
        out["strength_A"][:], out["strength_b"][:], out["strength_x"][:] = self.sA.ravel(), self.sb, self.sx
        out["strength_total"], out["strength_num_equations"] = self.total, self.num_equations


def ar_solve(S, is_chroma, cov):
    """ar_equation_system_solve (:992-1028)"""
    ret = linsolve(S.n, S.A.copy(), S.b.copy(), S.x, cov)
    S.ar_gain = np.float64(1.0)
    if not ret:
        return 0
    n, m = S.n, S.n - is_chroma
    var = np.float64(0)
    for i in range(m):
        var += S.A[i, i] / np.float64(S.num_observations)
    var /= np.float64(m)
    sum_covar = np.float64(0)
    for i in range(m):
        bi = S.b[i]
        if is_chroma:
            bi = bi - S.A[i, n - 1] * S.x[n - 1]
        sum_covar += (bi * S.x[i]) / np.float64(S.num_observations)
    d = var - sum_covar
    noise_var = d if d > 1e-6 else np.float64(1e-6)
    r = var / noise_var
    g = np.sqrt(r if r > 1e-6 else np.float64(1e-6))
    S.ar_gain = np.float64(1.0) if 1 > g else g
    return 1


def chroma_fallback(S):
    """set_chroma_coefficient_fallback_soln (:238-247)"""
    S.x[:] = 0
    if abs(S.A[-1, -1]) > 1e-6:
        S.x[-1] = S.b[-1] / S.A[-1, -1]


def bin_index(value, max_intensity):
    val = np.float64(min(max(value, 0.0), max_intensity))
    return (np.float64(BINS - 1) * (val - 0.0)) / np.float64(max_intensity - 0.0)


def strength_solve(S, cov):
    """aom_noise_strength_solver_solve (:314-350): mean / 8192 goes into the solver's own b on every call"""
    with np.errstate(all="ignore"):
        n = BINS
        k_alpha = np.float64(2.0) * np.float64(S.num_equations) / np.float64(n)
        A = S.sA.copy()
        for i in range(n):
            A[i, max(0, i - 1)] -= k_alpha
            A[i, i] += 2 * k_alpha
            A[i, min(n - 1, i + 1)] -= k_alpha
        mean = S.total / np.float64(S.num_equations)
        for i in range(n):
            A[i, i] += 1.0 / 8192.
            S.sb[i] += mean / 8192.
        return linsolve(n, A, S.sb.copy(), S.sx, cov)


# ---------------------------------------------------------------- aom_noise_model_update

def _observe(c, noise, w, h, flat, norm, cov):
    """add_block_observations (:818-883) of channel c -> A, b, the number of observations"""
    sub = int(c > 0)
    bs, pw, ph = BLOCK >> sub, w >> sub, h >> sub
    nbh, nbw = flat.shape
    n = COORDS + sub
    A, b, count = np.zeros((n, n)), np.zeros(n), 0
    N, Y = noise[c], noise[0]
    norm2 = np.float64(norm) * np.float64(norm)
    buf = np.zeros(n)
    for by in range(nbh):
        for bx in range(nbw):
            if not flat[by, bx]:
                continue
            x_o, y_o = bx * bs, by * bs
            y_start = 0 if by > 0 and flat[by - 1, bx] else LAG
            x_start = 0 if bx > 0 and flat[by, bx - 1] else LAG
            y_end = min(ph - by * bs, bs)
            right = bs if bx + 1 < nbw and flat[by, bx + 1] else bs - LAG
            x_end = min(pw - bx * bs - LAG, right)
            if cov is not None:
                cov["y_start_0" if y_start == 0 else "y_start_lag"] = cov["x_start_0" if x_start == 0 else "x_start_lag"] = True
                if x_end > x_start and y_end > y_start:
                    arm = "x_end_width" if pw - bx * bs - LAG < right else ("x_end_flat_right" if right == bs else "x_end_not_flat_right")
                    cov[arm] = True
                    cov["x_end_is_1"] = cov.get("x_end_is_1", False) or x_end == 1
            for y in range(y_start, y_end):
                for x in range(x_start, x_end):
                    X, Yy = x + x_o, y + y_o
                    buf[:COORDS] = N[Yy + CY, X + CX]
                    if sub:
                        buf[COORDS] = Y[2 * Yy:2 * Yy + 2, 2 * X:2 * X + 2].sum() / 4.0     # a sum of four integers: exact in any order
                    val = N[Yy, X]
                    A += np.outer(buf, buf) / norm2
                    b += (buf * val) / norm2
                    count += 1
    return A, b, count


def _strength_walk(c, st, data, noise, w, h, flat, top, cov):
    """add_noise_std_observations (:885-947) into st[c], luma's solved strength in st[0]"""
    S, L = st[c], st[0]
    sub = int(c > 0)
    bs, pw, ph = BLOCK >> sub, w >> sub, h >> sub
    nbh, nbw = flat.shape
    n = BINS
    with np.errstate(all="ignore"):
        for by in range(nbh):
            for bx in range(nbw):
                if not flat[by, bx]:
                    continue
                nw, nh = min(pw - bx * bs, bs), min(ph - by * bs, bs)
                if not nw * nh > BLOCK:
                    if cov is not None:
                        cov["gate_skips_block"] = True
                    continue
                if cov is not None and nw * nh < bs * bs and nh == bs:
                    cov["gate_keeps_narrow_column"] = True
                luma = data[0][by * BLOCK:by * BLOCK + BLOCK, bx * BLOCK:bx * BLOCK + BLOCK].astype(np.int64)
                block_mean = np.float64(int(luma.sum())) / np.float64(luma.size)
                nz = noise[c][by * bs:by * bs + nh, bx * bs:bx * bs + nw].astype(np.int64)
                noise_mean = np.float64(int(nz.sum())) / np.float64(nw * nh)
                noise_var = np.float64(int((nz * nz).sum())) / np.float64(nw * nh) - noise_mean * noise_mean
                luma_strength, corr = np.float64(0), np.float64(0)
                if c:
                    bin_ = bin_index(block_mean, top)
                    i0 = int(math.floor(bin_))
                    i1 = min(n - 1, i0 + 1)
                    a = bin_ - i0
                    luma_strength = L.ar_gain * ((1.0 - a) * L.sx[i0] + a * L.sx[i1])
                    corr = S.x[COORDS]
                cl = corr * luma_strength
                noise_std = np.sqrt(max(noise_var / 16, noise_var - cl * cl)) / S.ar_gain
                bin_ = bin_index(block_mean, top)
                i0 = int(math.floor(bin_))
                i1 = min(n - 1, i0 + 1)
                a = bin_ - i0
                S.sA[i0, i0] += (1.0 - a) * (1.0 - a)
                S.sA[i1, i0] += a * (1.0 - a)
                S.sA[i1, i1] += a * a
                S.sA[i0, i1] += a * (1.0 - a)
                S.sb[i0] += (1.0 - a) * noise_std
                S.sb[i1] += a * noise_std
                S.total += noise_std
                S.num_equations += 1


def noise_model(bd, data, den, flat, cov=None):
    """aom_noise_model_init + aom_noise_model_update -> the state (a 0-d array of STATE)"""
    h, w = data[0].shape
    top = (1 << bd) - 1
    latest = [Channel(COORDS + (c > 0)) for c in range(3)]
    combined = [Channel(COORDS + (c > 0)) for c in range(3)]
    noise = [d.astype(np.float64) - n.astype(np.float64) for d, n in zip(data, den)]

    def done(status):
        out = np.zeros((), STATE)
        for c in range(3):
            latest[c].pack(out["latest"][c]), combined[c].pack(out["combined"][c])
        out["status"] = status
        if cov is not None:
            cov[{OK: "status_ok", INSUFFICIENT: "status_insufficient", INTERNAL: "status_internal"}[status]] = True
        return out

    if np.count_nonzero(flat) <= 1:
        return done(INSUFFICIENT)
    for c in range(3):
        L, C = latest[c], combined[c]
        L.A, L.b, L.num_observations = _observe(c, noise, w, h, flat, top, cov)
        if not ar_solve(L, int(c > 0), cov):
            if not c:
                return done(INTERNAL)
            chroma_fallback(L)
            if cov is not None:
                cov["chroma_fallback"] = True
        _strength_walk(c, latest, data, noise, w, h, flat, top, cov)
        if not strength_solve(L, cov):
            return done(INTERNAL)
        C.num_observations = L.num_observations
        C.A, C.b, C.x = L.A.copy(), L.b.copy(), L.x.copy()
        if not ar_solve(C, int(c > 0), cov):
            if not c:
                return done(INTERNAL)
            chroma_fallback(C)
        C.sA, C.sb, C.sx, C.num_equations, C.total = L.sA.copy(), L.sb.copy(), L.sx.copy(), L.num_equations, L.total
        if not strength_solve(C, cov):
            return done(INTERNAL)
    return done(OK)


# ---------------------------------------------------------------- the flat-block finder

def flat_tables():
    """aom_flat_block_finder_init (:483-510): A[1024][3] then AtA_inv[3][3], flattened"""
    A = np.zeros((BLOCK * BLOCK, 3))
    ata = np.zeros((3, 3))
    for y in range(BLOCK):
        yd = (np.float64(y) - BLOCK / 2.) / (BLOCK / 2.)
        for x in range(BLOCK):
            xd = (np.float64(x) - BLOCK / 2.) / (BLOCK / 2.)
            A[y * BLOCK + x] = (yd, xd, 1)
            ata += np.outer(A[y * BLOCK + x], A[y * BLOCK + x])
    inv, xs = np.zeros((3, 3)), np.zeros(3)
    for i in range(3):
        b = np.zeros(3)
        b[i] = 1
        assert linsolve(3, ata.copy(), b, xs)
        inv[:, i] = xs
    return np.concatenate([A.ravel(), inv.ravel()])


def extract_block(luma, bd, offsx, offsy, tables):
    """aom_flat_block_finder_extract_block (:522-563) -> (plane, block), 1024 doubles each"""
    h, w = luma.shape
    A, inv = tables[:BLOCK * BLOCK * 3].reshape(-1, 3), tables[BLOCK * BLOCK * 3:].reshape(3, 3)
    ys, xs = np.minimum(offsy + np.arange(BLOCK), h - 1), np.minimum(offsx + np.arange(BLOCK), w - 1)
    block = (luma[np.ix_(ys, xs)].astype(np.float64) / np.float64((1 << bd) - 1)).ravel()
    ab = np.zeros(3)
    for i in range(BLOCK * BLOCK):
        ab += block[i] * A[i]
    pc = np.zeros(3)
    for c in range(3):
        pc += inv[:, c] * ab[c]
    plane = np.zeros(BLOCK * BLOCK)
    for c in range(3):
        plane += A[:, c] * pc[c]
    return plane, block - plane


def block_features(block):
    """:624-657 and the thresholds of :655-657, :670 on an extracted block -> (trace, ratio, norm, var), is_flat"""
    B = block.reshape(BLOCK, BLOCK)
    acc = np.zeros(5)
    t = np.zeros(5)
    for yi in range(1, BLOCK - 1):
        for xi in range(1, BLOCK - 1):
            gx, gy = (B[yi, xi + 1] - B[yi, xi - 1]) / 2, (B[yi + 1, xi] - B[yi - 1, xi]) / 2
            t[:] = gx * gx, gx * gy, gy * gy, B[yi, xi], B[yi, xi] * B[yi, xi]
            acc += t
    m = np.float64((BLOCK - 2) * (BLOCK - 2))
    Gxx, Gxy, Gyy, mean = acc[0] / m, acc[1] / m, acc[2] / m, acc[3] / m
    var = acc[4] / m - mean * mean
    trace, det = Gxx + Gyy, Gxx * Gyy - Gxy * Gxy
    with np.errstate(all="ignore"):
        root = np.sqrt(trace * trace - 4 * det)
    e1, e2 = (trace + root) / 2., (trace - root) / 2.
    ratio = e1 / (e2 if e2 > 1e-6 else np.float64(1e-6))
    is_flat = trace < 0.15 / (32 * 32) and ratio < 1.25 and e1 < 0.08 / (32 * 32) and var > 0.005 / np.float64(BLOCK * BLOCK)
    return (trace, ratio, e1, var), 255 if is_flat else 0


def flat_block_features(luma, bd, tables=None):
    """what svthip_[highbd_]film_grain_flat_block_features_dev writes: features (blocks,) of FEATURES and the is_flat bytes"""
    tables = flat_tables() if tables is None else tables
    h, w = luma.shape
    nbw, nbh = blocks_of(w, h)
    feat, flat = np.zeros(nbw * nbh, FEATURES), np.zeros(nbw * nbh, np.uint8)
    for b in range(nbw * nbh):
        _, block = extract_block(luma, bd, (b % nbw) * BLOCK, (b // nbw) * BLOCK, tables)
        (feat[b]["trace"], feat[b]["ratio"], feat[b]["norm"], feat[b]["var"]), flat[b] = block_features(block)
    return feat, flat


def finish_flat_blocks(feat, is_flat):
    """the host's part of aom_flat_block_finder_run behind the features (:665-698): the float score, the sort and the union with the top
    decile -> the final map, the scores and the threshold"""
    weights = (-6682, -0.2056, 13087, -12434, 2.5694)
    scores = np.zeros(len(feat), np.float32)
    for i, f in enumerate(feat):
        s = weights[0] * float(f["var"]) + weights[1] * float(f["ratio"]) + weights[2] * float(f["trace"]) + weights[3] * float(f["norm"]) + weights[4]
        score = np.float32(1.0 / (1 + (math.exp(-s) if -s < 709 else math.inf)))
        scores[i] = score if f["var"] > 0.005 / np.float64(BLOCK * BLOCK) else 0
    threshold = np.sort(scores)[len(feat) * 90 // 100]
    out = is_flat.copy()
    out[scores >= threshold] |= 1
    return out, scores, threshold
