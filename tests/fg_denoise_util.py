"""Film-grain Wiener denoising restated in numpy (TEST INFRASTRUCTURE): aom_wiener_denoise_2d (Codec/noise_model.c:1363-1500) with the block
extraction at any offset and at block size 32 or 16, the half-cosine window from the committed table, aom_fft_2d_gen / aom_ifft_2d_gen
(Codec/fft.c) over the 1-D networks of Codec/fft_common.h restated as the recursion they unroll from, aom_noise_tx_filter / _inverse
(Codec/noise_util.c), the overlapped accumulation and the serial dither.  float32 and float64 throughout: an elementwise numpy operation
is the IEEE operation, no sum is left to np.sum / np.dot, and everything whose order matters is sequential.  Blocks of one pass are
independent of each other and are carried as a trailing axis.

Also the pictures, contents, spectra and cases of tests/golden/fg_denoise.npz, and the counters (COVERAGE_KEYS) by which the generator
asserts what the cases reach."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tools")]

import fg_model_util as mu  # noqa: E402
import gen_fg_cos_window  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "fg_denoise.npz")
BLOCK = 32
F32, F64 = np.float32, np.float64
ZERO = F32(0)
NOISE_LEVEL = 5.0
COVERAGE_KEYS = ("filter_gain", "filter_floor", "filter_floor_by_eps_alone", "clamp_low", "clamp_high", "offset_negative_x", "offset_negative_y",
                 "offset_past_x", "offset_past_y")

# (width, height, bit depth); the first three are fg_model_util's, so the chain can use its planes
PICTURES = ((64, 64, 8), (100, 72, 8), (96, 40, 10), (36, 66, 8))
# (picture, content, psd)
CASES = ((0, "noisy", "default"), (0, "constant", "zero"), (0, "extremes", "default"), (0, "noisy", "nonflat"),
         (1, "noisy", "default"), (1, "extremes", "nonflat"), (1, "constant", "default"),
         (2, "noisy", "default"), (2, "extremes", "nonflat"), (2, "noisy", "zero"),
         (3, "noisy", "nonflat"), (3, "extremes", "default"))


def planes_of(p, content="noisy"):
    """the three data planes of picture p"""
    w, h, bd = PICTURES[p]
    top, dt = (1 << bd) - 1, np.uint16 if bd > 8 else np.uint8
    if content == "noisy":
        if p < len(mu.PICTURES):
            return mu.planes_of(p)[0]
        return mu.make_planes(w, h, bd, np.random.default_rng([11, p]))[0]
    rng = np.random.default_rng([23, p])
    out = []
    for k in range(3):
        ph, pw = h >> (k > 0), w >> (k > 0)
        if content == "constant":
            out.append(np.full((ph, pw), (97 + 30 * k) << (bd - 8), dt))
        else:
            assert content == "extremes"   # samples 0 and max in runs of random length, some mid-range texture between them
            v = np.where(rng.random((ph, pw)) < 0.5, 0, top)
            mid = rng.integers(0, top + 1, (ph, pw))
            out.append(np.where(rng.random((ph, pw)) < 0.2, mid, v).astype(dt))
    return out


def psd_default(block_size, factor):
    """aom_noise_psd_get_default_value (Codec/noise_util.c:25) in float as written"""
    f = F32(factor)
    return ((f * f / F32(10000)) * F32(block_size)) * F32(block_size) / F32(8)


def psd_of(kind, seed=0):
    """[Y 1024, Cb 1024, Cr 1024] floats as the reference takes them (chroma reads the first 256)"""
    out = []
    for c in range(3):
        n = BLOCK >> (c > 0)
        if kind == "default":
            a = np.full(BLOCK * BLOCK, psd_default(n, NOISE_LEVEL), F32)
        elif kind == "zero":
            a = np.zeros(BLOCK * BLOCK, F32)
        else:
            assert kind == "nonflat"   # grows along x much faster than along y: a transposed spectrum meets another threshold
            i = np.arange(BLOCK * BLOCK)
            y, x = i // n, i % n
            a = (psd_default(n, NOISE_LEVEL) * (F32(0.05) + F32(0.4) * x.astype(F32) + F32(0.01) * y.astype(F32) + F32(0.003) * ((i * 7 + seed + c) % 11).astype(F32))).astype(F32)
        out.append(np.ascontiguousarray(a))
    return out


def fixture():
    return np.load(FIXTURE)


# ---------------------------------------------------------------- tables, window, extraction

_TABLES = {}


def tables(n):
    """aom_flat_block_finder_init (:483-510) at block size n: A[n n][3], AtA_inv[3][3]"""
    if n not in _TABLES:
        A = np.zeros((n * n, 3))
        ata = np.zeros((3, 3))
        for y in range(n):
            yd = (F64(y) - n / 2.) / (n / 2.)
            for x in range(n):
                xd = (F64(x) - n / 2.) / (n / 2.)
                A[y * n + x] = (yd, xd, 1)
                ata += np.outer(A[y * n + x], A[y * n + x])
        inv, xs = np.zeros((3, 3)), np.zeros(3)
        for i in range(3):
            b = np.zeros(3)
            b[i] = 1
            assert mu.linsolve(3, ata.copy(), b, xs)
            inv[:, i] = xs
        _TABLES[n] = (A, inv)
    return _TABLES[n]


def window(n):
    """get_half_cos_window (:1314-1326): (float)(cos_y * cos_x) of the committed doubles, n x n"""
    t = np.array(gen_fg_cos_window.read_table())
    c = t[:32] if n == 32 else t[32:]
    assert len(c) == n
    return (c[:, None] * c[None, :]).astype(F32)


def extract_blocks(plane, bd, n, origins, cov=None):
    """aom_flat_block_finder_extract_block (:522-563) at block size n for every (ox, oy) of `origins` -> plane fits and residual blocks, (n n, blocks)
    doubles each"""
    h, w = plane.shape
    A, inv = tables(n)
    ox = np.array([o[0] for o in origins])
    oy = np.array([o[1] for o in origins])
    if cov is not None:
        cov["offset_negative_x"] |= bool((ox < 0).any())
        cov["offset_negative_y"] |= bool((oy < 0).any())
        cov["offset_past_x"] |= bool((ox + n > w).any())
        cov["offset_past_y"] |= bool((oy + n > h).any())
    i = np.arange(n * n)
    ys = np.clip(oy[None, :] + (i // n)[:, None], 0, h - 1)
    xs = np.clip(ox[None, :] + (i % n)[:, None], 0, w - 1)
    block = plane[ys, xs].astype(F64) / F64((1 << bd) - 1)
    ab = np.zeros((3, len(origins)))
    for k in range(n * n):
        ab += block[k][None, :] * A[k][:, None]
    pc = np.zeros((3, len(origins)))
    for c in range(3):
        pc += inv[:, c][:, None] * ab[c][None, :]
    fit = np.zeros_like(block)
    for c in range(3):
        fit += A[:, c][:, None] * pc[c][None, :]
    return fit, block - fit


# ---------------------------------------------------------------- the 1-D networks

TW = [F32(v) for v in (1.0, 0.980785, 0.92388, 0.83147, 0.707107, 0.55557, 0.382683, 0.19509, 0.0)]


def _fwd(x):
    """the forward network on x[N, ...] (real) -> R[0..N/2], I[0..N/2) (I[0] unused), B with I[N/4] = 0 - B"""
    N = len(x)
    if N == 4:
        w0, w1, w2, w3 = x[0] + x[2], x[0] - x[2], x[1] + x[3], x[1] - x[3]
        return [w0 + w2, w1, w0 - w2], [None, ZERO - w3], w3
    H, Q, E8 = N // 2, N // 4, N // 8
    er, ei, eb = _fwd(x[0::2])
    orr, oi, ob = _fwd(x[1::2])
    R, I = [None] * (H + 1), [None] * H
    R[0], R[H], R[Q] = er[0] + orr[0], er[0] - orr[0], er[Q]
    B = orr[Q]
    I[Q] = ZERO - B
    k2 = TW[4]
    md, ms = k2 * (orr[E8] - ob), k2 * (ob + orr[E8])
    R[E8], I[E8], R[H - E8], I[H - E8] = er[E8] + md, (ZERO - eb) - ms, er[E8] - md, eb - ms
    for k in range(1, Q):
        if k == E8:
            continue
        c, s = TW[k * 32 // N], TW[8 - k * 32 // N]
        cr, si, ci, sr = c * orr[k], s * oi[k], c * oi[k], s * orr[k]
        R[k], I[k] = er[k] + (cr + si), ei[k] + (ci - sr)
        R[H - k], I[H - k] = er[k] + ((ZERO - cr) - si), (ZERO - ei[k]) - (sr - ci)
    return R, I, B


def fft1d(x):
    """aom_fft1d_N along axis 0 of a float32 array: real parts 0..N/2, then the imaginary parts of 1..N/2-1"""
    R, I, _ = _fwd([x[i] for i in range(len(x))])
    return np.stack(R + I[1:])


def _inv(inp, N, M, O):
    """the M values Z[O + j N / M] of the inverse network's complex transform -> (re[M], im[M])"""
    H = N // 2
    if M == 2:
        if O == 0:
            return [inp[0] + inp[H], inp[0] - inp[H]], [None, None]
        ra, A, rb, Bv = inp[O], inp[H + O], inp[H - O], inp[N - O]
        return [ra + rb, ra - rb], [Bv - A, (ZERO - A) - Bv]
    h, Q = M // 2, M // 4
    er, ei = _inv(inp, N, h, O)
    orr, oi = _inv(inp, N, h, O + N // M)
    re, im = [None] * M, [None] * M
    if M == 4 and O == 0:
        re[0], im[0] = er[0] + orr[0], oi[0]
        re[2], im[2] = er[0] - orr[0], ZERO - oi[0]
        re[1], im[1] = er[1] + oi[1], ZERO - orr[1]
        re[3], im[3] = er[1] - oi[1], orr[1]
        return re, im
    k2 = TW[4]
    for q in range(h):
        j = q * 32 // M
        a, b, p, r = er[q], ei[q], orr[q], oi[q]
        if q == 0:
            re[q], im[q], re[q + h], im[q + h] = a + p, b + r, a - p, b - r
        elif q == Q:
            re[q], im[q], re[q + h], im[q + h] = a + r, b - p, a - r, b + p
        elif 2 * q == Q:
            re[q], im[q] = a + k2 * (p + r), b + k2 * (r - p)
            re[q + h], im[q + h] = a + ((ZERO - k2 * p) - k2 * r), b + k2 * (p - r)
        elif 2 * q == 3 * Q:
            re[q], im[q] = a - k2 * (p - r), b - k2 * (r + p)
            re[q + h], im[q + h] = a + k2 * (p - r), b + k2 * (r + p)
        elif q < Q:
            c, s = TW[j], TW[8 - j]
            re[q], im[q] = a + (c * p + s * r), b + (c * r - s * p)
            re[q + h], im[q + h] = a + ((ZERO - c * p) - s * r), b + (s * p - c * r)
        else:
            c, s = TW[16 - j], TW[j - 8]
            re[q], im[q] = a - (c * p - s * r), b + ((ZERO - c * r) - s * p)
            re[q + h], im[q + h] = a + (c * p - s * r), b + (c * r + s * p)
    return re, im


def ifft1d(x):
    """aom_ifft1d_N along axis 0"""
    N = len(x)
    re, _ = _inv([x[i] for i in range(N)], N, N, 0)
    return np.stack(re)


# ---------------------------------------------------------------- the 2-D transforms and the filter

def fft2d(block):
    """aom_fft_2d_gen on block[n, n, ...] -> the spectrum (re, im) as [n, n/2 + 1, ...] each: the columns it writes"""
    n = block.shape[0]
    H = n // 2
    out1 = fft1d(block)                                     # columns: out1[k, x]
    out2 = fft1d(np.swapaxes(out1, 0, 1))                   # temp = out1', its columns: out2[k, x]
    t = np.swapaxes(out2, 0, 1)                             # temp2[y, x], unpack_2d_output's col_fft
    re, im = np.zeros((n, H + 1) + block.shape[2:], F32), np.zeros((n, H + 1) + block.shape[2:], F32)
    # aom_fft_unpack_2d_output_sse2 (ASM_SSE2/fft_sse2.c:38-104), the form the AVX2 transform is given: at the edge rows and columns a
    # value is copied, not added to a zero, which matters at a negative zero
    for y in range(H + 1):
        y2, ye = y + H, 0 < y < H
        for x in range(H + 1):
            x2, xe = x + H, 0 < x < H
            v = t[y, x]
            if xe and ye:
                re[y, x], im[y, x] = v - t[y2, x2], t[y2, x] + t[y, x2]
                re[n - y, x], im[n - y, x] = v + t[y2, x2], -t[y2, x] + t[y, x2]
            elif ye:
                re[y, x], im[y, x] = v, t[y2, x]
                re[n - y, x], im[n - y, x] = v, -t[y2, x]
            else:
                re[y, x], im[y, x] = v, (t[y, x2] if xe else ZERO)
    return re, im


def tx_filter(re, im, psd, cov=None):
    """aom_noise_tx_filter (Codec/noise_util.c:93-112) on the columns 0..n/2; psd is the reference's array, row pitch n"""
    n = re.shape[0]
    k_beta, k_eps = F32(1.1), F32(1e-6)
    ps = psd[:n * n].reshape(n, n)[:, :n // 2 + 1].reshape((n, n // 2 + 1) + (1,) * (re.ndim - 2))
    with np.errstate(all="ignore"):
        p = re * re + im * im
        over = p > k_beta * ps
        gain_arm = over & (p.astype(F64) > 1e-6)
        gain = (p - ps) / np.where(p > k_eps, p, k_eps)
        floor = (k_beta - F32(1.0)) / k_beta
        g = np.where(gain_arm, gain, floor).astype(F32)
    if cov is not None:
        cov["filter_gain"] |= bool(gain_arm.any())
        cov["filter_floor"] |= bool((~gain_arm).any())
        cov["filter_floor_by_eps_alone"] |= bool((over & ~gain_arm).any())
    return re * g, im * g


def ifft2d(re, im):
    """aom_ifft_2d_gen (Codec/fft.c:114-184) with vec_size 8 on the spectrum's columns 0..n/2 -> [n, n, ...]"""
    n = re.shape[0]
    H = n // 2
    out = np.zeros((n, n) + re.shape[2:], F32)
    out[:H + 1, 0], out[:H + 1, 1] = re[:H + 1, 0], re[:H + 1, H]
    out[H + 1:, 0], out[H + 1:, 1] = im[1:H, 0], im[1:H, H]
    out[:, 2:H + 1] = re[:, 1:H]
    out[:, H + 1:] = im[:, 1:H]
    temp = np.zeros_like(out)
    temp[:, :2] = ifft1d(out[:, :2])
    temp[:, 2:] = fft1d(out[:, 2:])
    o2 = np.zeros_like(out)
    o2[0], o2[H] = temp[:, 0], temp[:, 1]
    for y in range(1, H):
        for x in range(n):
            mid = 0 < x < H
            if x <= H:
                o2[y, x] = temp[x, y + 1] + (temp[x + H, y + H] if mid else ZERO)
                o2[y + H, x] = temp[x, y + H] - (temp[x + H, y + 1] if mid else ZERO)
            else:
                o2[y, x] = temp[n - x, y + 1] - temp[n - x + H, y + H]
                o2[y + H, x] = temp[n - x + H, y + 1] + temp[n - x, y + H]
    return np.swapaxes(ifft1d(o2), 0, 1)


def tx_block(block, psd, cov=None):
    """aom_noise_tx_forward, _filter, _inverse on block[n, n, ...]"""
    n = block.shape[0]
    re, im = fft2d(block)
    re, im = tx_filter(re, im, psd, cov)
    return ifft2d(re, im) / F32(n * n)


# ---------------------------------------------------------------- the picture

def result_geometry(w, h):
    """(pitch, rows) of the reference's `result`"""
    return ((w + BLOCK - 1) // BLOCK + 2) * BLOCK, ((h + BLOCK - 1) // BLOCK + 2) * BLOCK


def wiener_filter(data, bd, psd, cov=None):
    """the four passes of aom_wiener_denoise_2d for the three planes -> three float planes in the reference's `result` geometry"""
    h, w = data[0].shape
    nbw, nbh = (w + BLOCK - 1) // BLOCK, (h + BLOCK - 1) // BLOCK
    pitch, rows = result_geometry(w, h)
    out = []
    for c in range(3):
        n = BLOCK >> (c > 0)
        win = window(n)
        result = np.zeros((rows, pitch), F32)
        for offsy in (0, n // 2):
            for offsx in (0, n // 2):
                origins = [(bx * n + offsx, by * n + offsy) for by in range(-1, nbh) for bx in range(-1, nbw)]
                fit, res = extract_blocks(data[c], bd, n, origins, cov)
                block = res.astype(F32).reshape(n, n, -1) * win[:, :, None]
                block = tx_block(block, psd[c], cov)
                plane = fit.astype(F32).reshape(n, n, -1) * win[:, :, None]
                add = (block + plane) * win[:, :, None]
                for k, (ox, oy) in enumerate(origins):
                    result[oy + n:oy + 2 * n, ox + n:ox + 2 * n] += add[:, :, k]
        out.append(result)
    return out


def dither(result, w, h, bd, cov=None):
    """dither_and_quantize (:1328-1361) of the three planes, sequential; the float planes are consumed"""
    norm = F32((1 << bd) - 1)
    k16, half = F32(16.0), F32(0.5)
    out = []
    with np.errstate(all="ignore"):
        for c in range(3):
            n, pw, ph = BLOCK >> (c > 0), w >> (c > 0), h >> (c > 0)
            r = result[c][n:n + ph + 1, n:n + pw + 1].copy()
            den = np.zeros((ph, pw), np.uint16 if bd > 8 else np.uint8)
            for y in range(ph):
                for x in range(pw):
                    v = r[y, x] * norm + half
                    lo = v if v > 0 else ZERO
                    cl = lo if lo < norm else norm
                    if cov is not None:
                        cov["clamp_low"] |= not v > 0
                        cov["clamp_high"] |= not lo < norm
                    q = int(cl)
                    err = -(F32(q) / norm - r[y, x])
                    den[y, x] = q
                    if x + 1 < pw:
                        r[y, x + 1] += err * F32(7.0) / k16
                    if y + 1 < ph:
                        if x > 0:
                            r[y + 1, x - 1] += err * F32(3.0) / k16
                        r[y + 1, x] += err * F32(5.0) / k16
                        if x + 1 < pw:
                            r[y + 1, x + 1] += err * F32(1.0) / k16
            out.append(den)
    return out


def denoise(data, bd, psd, cov=None):
    """aom_wiener_denoise_2d -> (the float planes before the dither, the denoised planes)"""
    h, w = data[0].shape
    planes = wiener_filter(data, bd, psd, cov)
    return planes, dither(planes, w, h, bd, cov)


def picture_area(planes, w, h):
    """the defined part of the three float planes, as uint32 bits"""
    return [np.ascontiguousarray(planes[c][(BLOCK >> (c > 0)):(BLOCK >> (c > 0)) + (h >> (c > 0)), (BLOCK >> (c > 0)):(BLOCK >> (c > 0)) + (w >> (c > 0))]).view(np.uint32)
            for c in range(3)]


def digest(a):
    """SHA-256 of an array's bytes, as 32 uint8"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def new_coverage():
    return {k: False for k in COVERAGE_KEYS}
