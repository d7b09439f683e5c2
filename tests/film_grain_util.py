"""TEST INFRASTRUCTURE ONLY -- AV1 film-grain synthesis of include/svtav1_hip.h (svthip_film_grain_tables_dev,
svthip_av1_[highbd_]add_film_grain_dev) restated with numpy integers from the reference's av1_add_film_grain_run
(Codec/grainSynthesis.c:995-1382): the shift register (:441-463), the luma and chroma templates with their autoregressive filter (:465-586),
init_scaling_function and scale_LUT (:588-623), the block offsets (:1089-1103), the overlap blends (:931-991 as the picture walk uses them)
and add_noise_to_block[_hbd] (:625-843).  4:2:0 only, 8 and 10 bits.  The frame pass is a pure function of the un-noised source: the grain
of a sample depends on the template offsets of at most four 32x32 blocks, and is put together per block with array operations.
tests/golden/make_golden_film_grain.py asserts it equal to the reference while it writes tests/golden/film_grain.npz;
tests/test_film_grain_vs_ref.py, tests/test_film_grain_kernels_host.py and tests/test_film_grain_gpu.py compare against it and the fixture.

The reference is NEVER run with num_y_points == 0: its dealloc_arrays (:402-438) then frees one pointer more than init_arrays (:306-400)
allocated.  Such parameter sets (REFERENCE_UNSAFE) are checked against this restatement only."""
import hashlib
import os
import struct
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tools")]
from gen_film_grain_gauss import GAUSS  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "film_grain.npz")
LUMA_H, LUMA_W, CHROMA_H, CHROMA_W = 73, 82, 38, 44
TABLE_PARTS = (("luma", LUMA_H * LUMA_W), ("cb", CHROMA_H * CHROMA_W), ("cr", CHROMA_H * CHROMA_W), ("scaling", 3 * 256))
TABLES_INT16 = sum(n for _, n in TABLE_PARTS)
# width, height: one block; all four overlap kinds; a block whose neighbours are blended themselves; cut blocks; a last block that is the
# overlap strip only, each way; partial blocks on both edges
SIZES = ((32, 32), (64, 64), (96, 96), (72, 40), (66, 34), (34, 66), (136, 72))
BIG = (1920, 1080)      # once, 8 bits, parameter set BIG_SET: 60 draws a row, 34 row seeds
BIG_SET = 4
BIT_DEPTHS = (8, 10)

# svthip_film_grain_params == aom_film_grain_t (Codec/grainSynthesis.h:29-81): name, int32 count; then uint16 random_seed, uint16 reserved
FIELDS = (("apply_grain", 1), ("update_parameters", 1), ("scaling_points_y", 28), ("num_y_points", 1), ("scaling_points_cb", 20), ("num_cb_points", 1),
          ("scaling_points_cr", 20), ("num_cr_points", 1), ("scaling_shift", 1), ("ar_coeff_lag", 1), ("ar_coeffs_y", 24), ("ar_coeffs_cb", 25),
          ("ar_coeffs_cr", 25), ("ar_coeff_shift", 1), ("cb_mult", 1), ("cb_luma_mult", 1), ("cb_offset", 1), ("cr_mult", 1), ("cr_luma_mult", 1),
          ("cr_offset", 1), ("overlap_flag", 1), ("clip_to_restricted_range", 1), ("bit_depth", 1), ("chroma_scaling_from_luma", 1),
          ("grain_scale_shift", 1))
PARAMS_BYTES = 4 * sum(n for _, n in FIELDS) + 4


def pack_params(p):
    """the parameter block as the C struct's bytes, built here independently of the package's film_grain_params()"""
    out = b""
    for name, n in FIELDS:
        v = np.zeros(n, np.int32)
        src = np.asarray(p.get(name, 0), np.int32).reshape(-1)
        v[:src.size] = src
        out += v.tobytes()
    return out + struct.pack("<HH", p["random_seed"], 0)


# ------------------------------------------------------------------------------------------------ parameter sets

def _points(xs, ys):
    return [[x, y] for x, y in zip(xs, ys)]


def _coeffs(seed, lag, lo, hi, luma_term=None):
    """AR coefficients of the three planes: 2 lag (lag + 1) each, Cb and Cr one more (the luma term, used when luma has points)"""
    rng = np.random.default_rng(seed)
    n = 2 * lag * (lag + 1)
    y, cb, cr = (rng.integers(lo, hi + 1, 25).tolist() for _ in range(3))
    if luma_term is not None:
        cb[n], cr[n] = luma_term
    return {"ar_coeffs_y": y[:24], "ar_coeffs_cb": cb, "ar_coeffs_cr": cr}


def _set(seed, lag, overlap, clip, csfl, gss, sshift, ar_shift, y, cb, cr, coeffs, mults=(128, 192, 256, 100, 160, 300)):
    p = {"apply_grain": 1, "update_parameters": 1, "random_seed": seed, "ar_coeff_lag": lag, "overlap_flag": overlap, "clip_to_restricted_range": clip,
         "chroma_scaling_from_luma": csfl, "grain_scale_shift": gss, "scaling_shift": sshift, "ar_coeff_shift": ar_shift,
         "scaling_points_y": y, "num_y_points": len(y), "scaling_points_cb": cb, "num_cb_points": len(cb), "scaling_points_cr": cr,
         "num_cr_points": len(cr), "bit_depth": 0}
    p.update(coeffs)
    p["cb_mult"], p["cb_luma_mult"], p["cb_offset"], p["cr_mult"], p["cr_luma_mult"], p["cr_offset"] = mults
    return p


_Y14 = _points((0, 10, 25, 40, 64, 90, 110, 128, 150, 180, 200, 220, 240, 255), (20, 90, 40, 160, 30, 255, 0, 80, 200, 60, 140, 10, 250, 120))
_C10 = _points((5, 30, 60, 90, 120, 150, 180, 210, 230, 250), (200, 20, 120, 60, 255, 0, 90, 180, 30, 140))
# Sets 0-2: lag 0, 10-bit templates at grain_scale_shift 0 are Gaussian entries / 4 (the chroma luma term is 0), and between them the three
# seeds draw every one of the 2 048 entries.  3, 5, 6: coefficients large enough to run the filter into its clamp.  7: no luma points
# (never given to the reference).  8, 9: a chroma plane without points.
PARAM_SETS = (
    _set(0x1234, 0, 1, 0, 0, 0, 8, 7, _points((128,), (96,)), _points((64,), (80,)), _points((200,), (255,)), _coeffs(1, 0, 0, 0, (0, 0))),
    _set(0xBEEF, 0, 0, 1, 1, 0, 11, 6, _points((40, 200), (255, 30)), _points((1,), (1,)), _points((2,), (2,)), _coeffs(2, 0, 0, 0, (0, 0))),
    _set(0x0001, 0, 1, 1, 0, 0, 9, 9, _Y14, _C10, _points((0, 255), (255, 0)), _coeffs(3, 0, 0, 0, (0, 0)), (255, 0, 511, 0, 255, 0)),
    _set(0x7A5C, 1, 1, 0, 0, 1, 8, 6, _points((0, 255), (255, 255)), _points((0, 128, 255), (255, 200, 255)), _points((10,), (255,)),
         _coeffs(4, 1, -128, 127)),
    _set(0xC0DE, 2, 1, 0, 0, 0, 10, 7, _Y14, _C10, _points((0, 100, 255), (40, 255, 90)), _coeffs(5, 2, -20, 20, (48, -40))),
    _set(0xFFFF, 3, 1, 0, 0, 2, 8, 7, _points((0, 255), (255, 255)), _points((0,), (255,)), _points((255,), (255,)), _coeffs(6, 3, -40, 45, (127, -128))),
    _set(0x0100, 3, 1, 1, 0, 0, 8, 6, _points((0, 255), (255, 255)), _points((0,), (255,)), _points((255,), (255,)), _coeffs(7, 3, -60, 60, (90, -90))),
    _set(0x5EED, 2, 1, 0, 0, 0, 9, 8, [], _C10, _points((50, 150), (255, 100)), _coeffs(8, 2, -25, 25)),
    _set(0x2468, 1, 1, 1, 0, 3, 11, 8, _points((0, 128, 255), (255, 128, 255)), [], _C10, _coeffs(9, 1, -30, 30, (60, 60))),
    _set(0x1357, 3, 0, 0, 1, 1, 10, 9, _points((16, 235), (100, 255)), _points((3,), (3,)), [], _coeffs(10, 3, -12, 12, (-100, 100))),
)
REFERENCE_UNSAFE = tuple(i for i, p in enumerate(PARAM_SETS) if p["num_y_points"] == 0)
# what the fixture keeps whole (the three planes the reference leaves) per size: (parameter set, bit depth); every other
# size x set x depth is kept as a digest of those planes.  AV1_WRAPPER cases went through av1_add_film_grain with bordered buffers.
KEPT = {0: ((0, 8), (3, 10)), 1: ((3, 8), (4, 10), (6, 8)), 2: ((5, 10), (2, 8)), 3: ((1, 8), (6, 10), (9, 10)), 4: ((8, 8), (5, 10), (2, 10)),
        5: ((4, 8), (0, 10), (9, 8)), 6: ((5, 8), (1, 10), (8, 10))}
AV1_WRAPPER = ((3, 4, 8), (6, 5, 10))    # size index, parameter set, bit depth


def source_planes(w, h, bit_depth, key):
    """the un-noised picture of a case: uniform samples over the whole range, with runs of the extreme values so that both sample clamps are met"""
    rng = np.random.default_rng([w, h, bit_depth, key])
    top = (1 << bit_depth) - 1
    dt = np.uint8 if bit_depth == 8 else np.uint16
    planes = []
    for ph, pw in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
        p = rng.integers(0, top + 1, (ph, pw))
        r = rng.integers(0, 8, (ph, pw))
        p = np.where(r == 0, rng.integers(0, 3, (ph, pw)), np.where(r == 1, top - rng.integers(0, 3, (ph, pw)), p))
        planes.append(p.astype(dt))
    return planes


def digest(planes):
    h = hashlib.blake2b(digest_size=8)
    for p in planes:
        h.update(np.ascontiguousarray(p).tobytes())
    return np.frombuffer(h.digest(), np.uint64)[0]


# ------------------------------------------------------------------------------------------------ the shift register

def lfsr_step(r):
    bit = (r ^ (r >> 1) ^ (r >> 3) ^ (r >> 12)) & 1
    return (r >> 1) | (bit << 15)


def row_seed(seed, luma_num):
    """init_random_generator (:450-463) for luma line 32 * luma_num"""
    return (seed ^ (((luma_num * 37 + 178) & 255) << 8) ^ ((luma_num * 173 + 105) & 255)) & 0xFFFF


def _draws(r, n, bits):
    out = np.zeros(n, np.int64)
    for i in range(n):
        r = lfsr_step(r)
        out[i] = (r >> (16 - bits)) & ((1 << bits) - 1)
    return out, r


# ------------------------------------------------------------------------------------------------ templates and scaling tables

def _grain_range(bit_depth):
    c = 128 << (bit_depth - 8)
    return -c, (256 << (bit_depth - 8)) - 1 - c


def _ar_filter(blk, coeffs, lag, shift, lo, hi, extra=None, extra_coeff=0, cov=None):
    """rows 3.., columns 3..W-4 in raster order, clamped at every sample; extra[i][j] * extra_coeff is the chroma luma term"""
    h, w = blk.shape
    n = 2 * lag * (lag + 1)
    ca = np.array(coeffs[:n - lag], np.int64).reshape(lag, 2 * lag + 1) if lag else None
    cl = np.array(coeffs[n - lag:n], np.int64)
    rnd = 1 << (shift - 1)
    for i in range(3, h):
        for j in range(3, w - 3):
            s = 0
            if lag:
                s = int((ca * blk[i - lag:i, j - lag:j + lag + 1]).sum()) + int((cl * blk[i, j - lag:j]).sum())
            if extra is not None:
                s += extra_coeff * int(extra[i, j])
            v = int(blk[i, j]) + ((s + rnd) >> shift)
            if cov is not None:
                cov["ar_clamp_low"] |= v < lo
                cov["ar_clamp_high"] |= v > hi
            blk[i, j] = min(max(v, lo), hi)


def scaling_function(points, n):
    """init_scaling_function (:588-609): integer division, 64-bit product, flat before the first and after the last point"""
    lut = np.zeros(256, np.int64)
    if n == 0:
        return lut
    lut[:points[0][0]] = points[0][1]
    for k in range(n - 1):
        dy, dx = points[k + 1][1] - points[k][1], points[k + 1][0] - points[k][0]
        delta = dy * ((65536 + (dx >> 1)) // dx)
        for x in range(dx):
            lut[points[k][0] + x] = points[k][1] + ((x * delta + 32768) >> 16)
    lut[points[n - 1][0]:] = points[n - 1][1]
    return lut


def tables(p, bit_depth, cov=None, drawn=None):
    """{"luma" [73][82], "cb", "cr" [38][44], "scaling" [3][256]} int16: the table block of svthip_film_grain_tables_dev.  A template of a
    plane without points is all zero (the device skips it; the reference leaves it uninitialised and never uses it)"""
    lo, hi = _grain_range(bit_depth)
    gshift = 12 - bit_depth + p["grain_scale_shift"]
    lag, ashift = p["ar_coeff_lag"], p["ar_coeff_shift"]
    n = 2 * lag * (lag + 1)
    gauss = np.array(GAUSS, np.int64)

    def template(r, hh, ww):
        idx, _ = _draws(r, hh * ww, 11)
        if drawn is not None:
            drawn[idx] = True
        return ((gauss[idx] + ((1 << gshift) >> 1)) >> gshift).reshape(hh, ww)

    out = {"luma": np.zeros((LUMA_H, LUMA_W), np.int64), "cb": np.zeros((CHROMA_H, CHROMA_W), np.int64), "cr": np.zeros((CHROMA_H, CHROMA_W), np.int64)}
    if p["num_y_points"]:
        out["luma"] = template(p["random_seed"], LUMA_H, LUMA_W)      # no row mix (:1014)
        _ar_filter(out["luma"], p["ar_coeffs_y"], lag, ashift, lo, hi, cov=cov)
    extra = None
    if p["num_y_points"]:
        L = out["luma"]
        extra = np.zeros((CHROMA_H, CHROMA_W), np.int64)
        # rows and columns ((i - 3) << 1) + 3, a rounded 2x2 mean (:551-566)
        extra[3:, 3:CHROMA_W - 3] = (L[3:73:2, 3:79:2] + L[3:73:2, 4:80:2] + L[4:74:2, 3:79:2] + L[4:74:2, 4:80:2] + 2)[:CHROMA_H - 3, :CHROMA_W - 6] >> 2
    for name, row, coeffs, pts in (("cb", 7, p["ar_coeffs_cb"], p["num_cb_points"]), ("cr", 11, p["ar_coeffs_cr"], p["num_cr_points"])):
        if pts:
            out[name] = template(row_seed(p["random_seed"], row), CHROMA_H, CHROMA_W)
            _ar_filter(out[name], coeffs, lag, ashift, lo, hi, extra, coeffs[n] if extra is not None else 0, cov=cov)
    sy = scaling_function(p["scaling_points_y"], p["num_y_points"])
    if p["chroma_scaling_from_luma"]:
        scb = scr = sy
    else:
        scb, scr = scaling_function(p["scaling_points_cb"], p["num_cb_points"]), scaling_function(p["scaling_points_cr"], p["num_cr_points"])
    out["scaling"] = np.stack([sy, scb, scr])
    return {k: v.astype(np.int16) for k, v in out.items()}


_TABLES = {}


def tables_of(s, bit_depth):
    """tables(PARAM_SETS[s], bit_depth), computed once per process"""
    if (s, bit_depth) not in _TABLES:
        _TABLES[(s, bit_depth)] = tables(PARAM_SETS[s], bit_depth)
    return _TABLES[(s, bit_depth)]


def tables_block(t):
    """the tables as the flat int16 block the header documents"""
    return np.concatenate([t[k].reshape(-1) for k, _ in TABLE_PARTS]).astype(np.int16)


def split_block(block):
    out, at = {}, 0
    shapes = {"luma": (LUMA_H, LUMA_W), "cb": (CHROMA_H, CHROMA_W), "cr": (CHROMA_H, CHROMA_W), "scaling": (3, 256)}
    for k, n in TABLE_PARTS:
        out[k] = np.asarray(block[at:at + n], np.int16).reshape(shapes[k])
        at += n
    return out


# ------------------------------------------------------------------------------------------------ the frame pass

def block_offsets(seed, w, h):
    """[block rows][block columns][2] = offset_y, offset_x nibbles: one 8-bit draw per block, each block row seeded by its index (:1089-1096)"""
    nby, nbx = (h + 31) // 32, (w + 31) // 32
    out = np.zeros((nby, nbx, 2), np.int64)
    for by in range(nby):
        d, _ = _draws(row_seed(seed, by), nbx, 8)
        out[by, :, 0], out[by, :, 1] = d & 15, (d >> 4) & 15
    return out


def grain_plane(T, offs, w, h, chroma, overlap, lo, hi, cov=None):
    """the grain of every sample of a w x h plane from template T: the block's template window, the left ov columns blended with the left
    neighbour's raw columns bs .. bs + ov - 1, the top ov rows blended with the rows bs .. of the strip-blended block above (:1105-1218)"""
    bs, ov = (16, 1) if chroma else (32, 2)
    wl, wr = (np.array([23]), np.array([22])) if chroma else (np.array([27, 17]), np.array([17, 27]))
    T = T.astype(np.int64)
    nby, nbx = offs.shape[:2]
    g = np.zeros((nby * bs, nbx * bs), np.int64)
    above = [None] * nbx
    for by in range(nby):
        left_raw = None
        for bx in range(nbx):
            oy, ox = (6 + offs[by, bx, 0], 6 + offs[by, bx, 1]) if chroma else (9 + 2 * offs[by, bx, 0], 9 + 2 * offs[by, bx, 1])
            raw = T[oy:oy + bs + ov, ox:ox + bs + ov]
            assert raw.shape == (bs + ov, bs + ov)
            hb = raw.copy()
            if overlap and bx:
                v = (wl * left_raw[:, bs:bs + ov] + wr * raw[:, :ov] + 16) >> 5
                if cov is not None:
                    cov["blend_clamp"] |= bool(((v < lo) | (v > hi)).any())
                hb[:, :ov] = np.clip(v, lo, hi)
            fin = hb[:bs, :bs].copy()
            if overlap and by:
                v = (wl[:, None] * above[bx][bs:bs + ov, :bs] + wr[:, None] * hb[:ov, :bs] + 16) >> 5
                if cov is not None:
                    cov["blend_clamp"] |= bool(((v < lo) | (v > hi)).any())
                fin[:ov] = np.clip(v, lo, hi)
            g[by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs] = fin
            above[bx], left_raw = hb, raw
    return g[:h, :w]


def _scale(lut, index, bit_depth, cov=None):
    lut = lut.astype(np.int64)
    if bit_depth == 8:
        return lut[index]
    x, frac = index >> 2, index & 3
    if cov is not None:
        cov["x255_arm"] |= bool((x == 255).any())
    nxt = lut[np.minimum(x + 1, 255)]
    return np.where(x == 255, lut[x], lut[x] + (((nxt - lut[x]) * frac + 2) >> 2))


def add_film_grain(p, bit_depth, luma, cb, cr, t=None, cov=None):
    """the three planes after av1_add_film_grain_run, from the un-noised planes (any integer dtype; the result has the luma's dtype)"""
    t = t or tables(p, bit_depth)
    h, w = luma.shape
    lo, hi = _grain_range(bit_depth)
    sh = bit_depth - 8
    top = (256 << sh) - 1
    offs = block_offsets(p["random_seed"], w, h)
    rnd, sshift = 1 << (p["scaling_shift"] - 1), p["scaling_shift"]
    if p["clip_to_restricted_range"]:
        ymin, ymax, cmin, cmax = 16 << sh, 235 << sh, 16 << sh, 240 << sh
    else:
        ymin = cmin = 0
        ymax = cmax = top
    Y = luma.astype(np.int64)
    out = [luma.copy(), cb.copy(), cr.copy()]

    def clamp(v, a, b, key):
        if cov is not None:
            cov[key + "_low"] |= bool((v < a).any())
            cov[key + "_high"] |= bool((v > b).any())
        return np.clip(v, a, b)

    key = "restricted_clamp" if p["clip_to_restricted_range"] else "full_clamp"
    if p["num_y_points"]:
        g = grain_plane(t["luma"], offs, w, h, False, p["overlap_flag"], lo, hi, cov)
        out[0] = clamp(Y + ((_scale(t["scaling"][0], Y, bit_depth, cov) * g + rnd) >> sshift), ymin, ymax, key).astype(luma.dtype)
    avg = (Y[0::2, 0::2] + Y[0::2, 1::2] + 1) >> 1
    for k, (plane, name, n) in enumerate(((cb, "cb", p["num_cb_points"]), (cr, "cr", p["num_cr_points"])), 1):
        if not n:
            continue
        if p["chroma_scaling_from_luma"]:
            mult, lmult, off = 0, 64, 0
        else:
            mult, lmult = p[name + "_mult"] - 128, p[name + "_luma_mult"] - 128
            off = (p[name + "_offset"] << sh) - (1 << bit_depth)    # 8 bits: offset - 256
        C = plane.astype(np.int64)
        g = grain_plane(t[name], offs, w // 2, h // 2, True, p["overlap_flag"], lo, hi, cov)
        index = np.clip(((avg * lmult + mult * C) >> 6) + off, 0, top)
        out[k] = clamp(C + ((_scale(t["scaling"][k], index, bit_depth, cov) * g + rnd) >> sshift), cmin, cmax, key).astype(plane.dtype)
    return out


# ------------------------------------------------------------------------------------------------ coverage

COVERAGE_KEYS = tuple(f"lag_{k}" for k in range(4)) + (
    "overlap_0", "overlap_1", "clip_0", "clip_1", "csfl_0", "csfl_1", "grain_scale_shift_0", "grain_scale_shift_above_0", "scaling_shift_8",
    "scaling_shift_11", "luma_points_1", "luma_points_2", "luma_points_14", "no_luma_points", "no_cb_points", "no_cr_points", "ar_clamp_low",
    "ar_clamp_high", "blend_clamp", "full_clamp_low", "full_clamp_high", "restricted_clamp_low", "restricted_clamp_high", "x255_arm", "interior",
    "left_strip", "top_strip", "corner", "cut_block", "strip_only_block", "every_gaussian_entry", "both_bit_depths")


def coverage(cases):
    """cases: (parameter set, bit depth, w, h) -> {key: reached}"""
    cov = {k: False for k in COVERAGE_KEYS}
    drawn = np.zeros(2048, bool)
    depths = set()
    done_tables = {}
    for p, bd, w, h in cases:
        depths.add(bd)
        cov[f"lag_{p['ar_coeff_lag']}"] = True
        for k, v in (("overlap", p["overlap_flag"]), ("clip", p["clip_to_restricted_range"]), ("csfl", p["chroma_scaling_from_luma"])):
            cov[f"{k}_{v}"] = True
        cov["grain_scale_shift_0"] |= p["grain_scale_shift"] == 0
        cov["grain_scale_shift_above_0"] |= p["grain_scale_shift"] > 0
        for s in (8, 11):
            cov[f"scaling_shift_{s}"] |= p["scaling_shift"] == s
        for n in (1, 2, 14):
            cov[f"luma_points_{n}"] |= p["num_y_points"] == n
        for k in ("y", "cb", "cr"):
            cov["no_luma_points" if k == "y" else f"no_{k}_points"] |= p[f"num_{k}_points"] == 0
        tk = (id(p), bd)
        if tk not in done_tables:
            pure = bd == 10 and p["ar_coeff_lag"] == 0 and p["grain_scale_shift"] == 0 and p["ar_coeffs_cb"][0] == 0 and p["ar_coeffs_cr"][0] == 0
            d = np.zeros(2048, bool)
            done_tables[tk] = tables(p, bd, cov, d)
            if pure:
                drawn |= d
        luma, cb, cr = source_planes(w, h, bd, PARAM_SETS.index(p) if p in PARAM_SETS else 0)
        add_film_grain(p, bd, luma, cb, cr, done_tables[tk], cov)
        if p["overlap_flag"] and p["num_y_points"]:
            cov["interior"] = True
            cov["left_strip"] |= w > 32
            cov["top_strip"] |= h > 32
            cov["corner"] |= w > 32 and h > 32
            cov["cut_block"] |= w % 32 not in (0, 2) or h % 32 not in (0, 2)
            cov["strip_only_block"] |= w % 32 == 2 or h % 32 == 2
    cov["every_gaussian_entry"] = bool(drawn.all())
    cov["both_bit_depths"] = depths == {8, 10}
    return {k: bool(v) for k, v in cov.items()}


def all_cases():
    """every (parameter set index, bit depth, size index) of the suite; size index len(SIZES) is BIG"""
    out = [(s, bd, z) for z in range(len(SIZES)) for s in range(len(PARAM_SETS)) for bd in BIT_DEPTHS]
    return out + [(BIG_SET, 8, len(SIZES))]


def size_of(z):
    return BIG if z == len(SIZES) else SIZES[z]


# ------------------------------------------------------------------------------------------------ the fixture

def fixture():
    """tests/golden/film_grain.npz:
      sizes [7][2], big [2]; params [10][PARAMS_BYTES] u8 (pack_params of PARAM_SETS)
      tables_s{set}_b{depth}     the reference's table block (int16, the header's layout) for every set the reference may be given
      digest [8][10][2] u64      blake2b-8 of the reference's three planes for size x set x depth (0 where it was not run)
      out_z{size}_s{set}_b{depth}_{y,cb,cr}   the reference's planes themselves for the combinations of KEPT and AV1_WRAPPER
      coverage_keys"""
    return np.load(FIXTURE)
