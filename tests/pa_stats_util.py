"""TEST INFRASTRUCTURE ONLY -- the picture-analysis statistics of include/svtav1_hip.h (svthip_pa_block_stats_dev, svthip_pa_homogeneity_dev,
svthip_pa_histograms_dev) restated with numpy integers from the reference's GatheringPictureStatistics
(Codec/EbPictureAnalysisProcess.c:4742-4796).  Takes the unpadded planes of a picture and clamps coordinates itself (np.pad mode "edge" is
the reference's replicated border).  tests/golden/make_golden_pa_stats.py asserts it equal to the reference while it writes
tests/golden/pa_stats.npz; tests/test_pa_stats_vs_ref.py, tests/test_pa_stats_kernels_host.py and tests/test_pa_stats_gpu.py compare against it
and against the fixture."""
import os

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "pa_stats.npz")
# width, height; every case at both precisions
CASES = ((64, 64), (136, 72), (72, 136), (200, 136), (320, 192))
OUTPUTS = ("y_mean", "variance", "cb_mean", "cr_mean", "var_of_var", "homogeneous", "picture", "histogram", "region_intensity", "average_intensity")
U64 = np.uint64


def sb_grid(w, h):
    return (w + 63) // 64, (h + 63) // 64


def complete_sbs(w, h):
    """[n_sb] bool, raster order: is_complete_sb"""
    nx, ny = sb_grid(w, h)
    return np.array([(x + 1) * 64 <= w and (y + 1) * 64 <= h for y in range(ny) for x in range(nx)])


def _leaf_tables(plane, nx, ny, sub):
    """8x8 leaves of a plane padded by replication to ny x nx blocks of 64: fixed-point mean (8.8) and mean of squares (16.16), [8 ny][8 nx]"""
    h, w = plane.shape
    p = np.pad(plane, ((0, ny * 64 - h), (0, nx * 64 - w)), mode="edge").astype(U64).reshape(ny * 8, 8, nx * 8, 8)
    rows = p[:, ::2] if sub else p
    return rows.sum((1, 3)) << U64(2 + sub), (rows * rows).sum((1, 3)) << U64(10 + sub)


def _up(a):
    return (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) >> U64(2)


def _per_sb(levels, nx, ny):
    """[ny k][nx k] tables, largest block first -> [n_sb][sum k^2] in ME_TIER_ZERO_PU order"""
    out = []
    for sy in range(ny):
        for sx in range(nx):
            out.append(np.concatenate([t[sy * k:(sy + 1) * k, sx * k:(sx + 1) * k].reshape(-1) for t in levels for k in (t.shape[0] // ny,)]))
    return np.array(out, U64)


def block_stats(luma, cb, cr, sub):
    """-> y_mean [n_sb][85] u8, variance [n_sb][85] u16, cb_mean, cr_mean [n_sb][21] u8"""
    h, w = luma.shape
    nx, ny = sb_grid(w, h)
    sub = int(bool(sub))
    m8, s8 = _leaf_tables(luma, nx, ny, sub)
    m16, s16 = _up(m8), _up(s8)
    m32, s32 = _up(m16), _up(s16)
    m64, s64 = _up(m32), _up(s32)
    m, s = _per_sb((m64, m32, m16, m8), nx, ny), _per_sb((s64, s32, s16, s8), nx, ny)
    with np.errstate(over="ignore"):
        variance = ((s - m * m) >> U64(16)).astype(np.uint16)       # unsigned 64-bit, wrapping as the reference's
    y_mean = (m >> U64(8)).astype(np.uint8)
    complete = complete_sbs(w, h)
    chroma = []
    for plane in (cb, cr):
        c16, _ = _leaf_tables(plane, (nx + 1) // 2, (ny + 1) // 2, sub)   # 8x8 chroma leaves = the "16x16" entries
        c16 = c16[:ny * 4, :nx * 4]
        c32 = _up(c16)
        t = _per_sb((c32[0::2, 0::2], c32, c16), nx, ny)                # [0] is replaced below
        q = t[:, 1:5]
        t[:, 0] = (q[:, 0] + q[:, 1] + q[:, 3] + q[:, 3]) >> U64(2)      # the reference's 64x64 chroma mean (:1926-1927)
        t[~complete] = 0
        chroma.append((t >> U64(8)).astype(np.uint8))
    return y_mean, variance, chroma[0], chroma[1]


def homogeneity(variance, w, h):
    """variance [n_sb][85] -> var_of_var [n_sb][4] u64, homogeneous [n_sb] u8, picture [4] u32"""
    n_sb = variance.shape[0]
    complete = complete_sbs(w, h)
    assert complete.any(), "no complete SB: the reference divides by zero"
    v8 = variance[:, 21:].astype(U64).reshape(n_sb, 8, 8)
    vov = np.full((n_sb, 4), ~U64(0), U64)
    homogeneous = np.ones(n_sb, np.uint8)
    for q in range(4):
        blk = v8[:, (q >> 1) * 4:(q >> 1) * 4 + 4, (q & 1) * 4:(q & 1) * 4 + 4].reshape(n_sb, 16)
        msq, mv = (blk * blk).sum(1) >> U64(4), blk.sum(1) >> U64(4)
        vov[complete, q] = (msq - mv * mv)[complete]
    flat = v8.reshape(n_sb, 64)
    msq, mv = (flat * flat).sum(1) >> U64(6), flat.sum(1) >> U64(6)
    homogeneous[complete & ((msq - mv * mv) > 64 * 64)] = 0
    v64 = variance[:, 0].astype(np.int64)
    pct = int((v64[complete] < 5).sum()) * 100 // int(complete.sum())
    picture = np.array([(int(v64.sum()) // n_sb) & 0xffff, pct > 60, pct > 80, complete.sum()], np.uint32)
    return vov, homogeneous, picture


def region_geometry(w, h, plane, rx, ry):
    """(x0, y0, columns visited, rows visited, step, rounding term, divisor) in samples of the plane read: the 1/16 luma plane, or a chroma plane"""
    pw, ph = (w, h) if plane else (w >> 2, h >> 2)
    rw, rh = pw // 4, ph // 4
    fw, fh = rw + (pw - 4 * rw if rx == 3 else 0), rh + (ph - 4 * rh if ry == 3 else 0)
    area = fw * fh
    if plane == 0:
        return rx * rw, ry * rh, fw, fh, 1, area >> 1, area
    return (rx * rw) >> 1, (ry * rh) >> 1, ((fw >> 1) + 3) // 4, ((fh >> 1) + 3) // 4, 4, area >> 3, area >> 2


def histograms(luma, cb, cr):
    """-> histogram [4][4][3][256] u32, region_intensity [4][4][3] u32, average_intensity [3] u32 (SCD_MODE_1)"""
    h, w = luma.shape
    planes = (luma[::4, ::4][:h >> 2, :w >> 2], cb, cr)
    hist = np.zeros((4, 4, 3, 256), np.uint32)
    region = np.zeros((4, 4, 3), np.uint32)
    total = [0, 0, 0]
    for rx in range(4):
        for ry in range(4):
            for p in range(3):
                x0, y0, cols, rows, step, rnd, div = region_geometry(w, h, p, rx, ry)
                v = planes[p][y0:y0 + rows * step:step, x0:x0 + cols * step:step]
                assert v.shape == (rows, cols), (v.shape, rows, cols)
                s = int(v.sum(dtype=np.int64))
                hist[rx, ry, p] = (1 + np.bincount(v.reshape(-1), minlength=256)) << 4
                region[rx, ry, p] = (((s << 4 if p else s) + rnd) // div) & 0xff
                total[p] += s << 4
    area = w * h
    avg = np.array([((total[0] + (area >> 1)) // area) & 0xff] + [((total[p] + (area >> 3)) // (area >> 2)) & 0xff for p in (1, 2)], np.uint32)
    return hist, region, avg


def all_stats(luma, cb, cr, sub):
    """every output of the three entries for one picture, keyed as OUTPUTS"""
    h, w = luma.shape
    y, v, b, r = block_stats(luma, cb, cr, sub)
    out = {"y_mean": y, "variance": v, "cb_mean": b, "cr_mean": r}
    if w >= 64 and h >= 64:
        out["var_of_var"], out["homogeneous"], out["picture"] = homogeneity(v, w, h)
    out["histogram"], out["region_intensity"], out["average_intensity"] = histograms(luma, cb, cr)
    return out


# ---------------------------------------------------------------------------------------------- the fixture

COVERAGE_KEYS = ("flat_0", "flat_255", "checkerboard_max_variance", "sub_differs_from_full", "incomplete_sb_right", "incomplete_sb_bottom",
                 "very_low_flag_0", "very_low_flag_1", "logo_flag_0", "logo_flag_1", "very_low_without_logo", "homogeneous_0", "homogeneous_1",
                 "var_of_var_all_ones", "chroma_quirk_matters", "last_region_wider", "last_region_higher", "odd_chroma_region_width",
                 "product_past_31_bits", "pyramid_truncates")


def coverage(cases):
    """cases: [(w, h, luma, cb, cr, {sub: outputs})] -> {key: reached}"""
    c = dict.fromkeys(COVERAGE_KEYS, False)
    for (w, h, luma, cb, cr, outs) in cases:
        full, sub = outs[0], outs[1]
        c["flat_0"] |= bool((luma == 0).all())
        c["flat_255"] |= bool((luma == 255).all())
        c["product_past_31_bits"] |= bool((luma == 255).all())        # m = 65280: m * m = 4261478400 > 2^31
        c["checkerboard_max_variance"] |= int(full["variance"].max()) == 16256
        c["sub_differs_from_full"] |= not np.array_equal(full["variance"], sub["variance"])
        c["incomplete_sb_right"] |= w % 64 != 0
        c["incomplete_sb_bottom"] |= h % 64 != 0
        if "picture" in full:
            for o in (full, sub):
                c[f"very_low_flag_{int(o['picture'][1])}"] = True
                c[f"logo_flag_{int(o['picture'][2])}"] = True
                c["very_low_without_logo"] |= bool(o["picture"][1]) and not bool(o["picture"][2])
                comp = complete_sbs(w, h)
                c["homogeneous_0"] |= bool((o["homogeneous"][comp] == 0).any())
                c["homogeneous_1"] |= bool((o["homogeneous"][comp] == 1).any())
                c["var_of_var_all_ones"] |= bool((o["var_of_var"] == ~U64(0)).any())
        nx, ny = sb_grid(w, h)
        m16, _ = _leaf_tables(cb, (nx + 1) // 2, (ny + 1) // 2, 0)
        plain = (_up(_up(m16[:ny * 4, :nx * 4])) >> U64(8)).reshape(-1)   # what a 64x64 chroma mean of all four 32x32 would be
        comp = complete_sbs(w, h)
        c["chroma_quirk_matters"] |= bool((plain[comp] != full["cb_mean"][comp, 0]).any())
        c["last_region_wider"] |= (w >> 2) % 4 != 0
        c["last_region_higher"] |= (h >> 2) % 4 != 0
        c["odd_chroma_region_width"] |= ((w // 4) >> 1) % 2 == 1
        m8, _ = _leaf_tables(luma, nx, ny, 0)
        m16 = _up(m8)                                                   # exact: the leaves carry two fraction bits more than their sums
        q = m16[0::2, 0::2] + m16[0::2, 1::2] + m16[1::2, 0::2] + m16[1::2, 1::2]
        c["pyramid_truncates"] |= bool((q & U64(3)).any())
    return c


_cache = {}


def fixture():
    if "z" not in _cache:
        _cache["z"] = dict(np.load(FIXTURE))
    return _cache["z"]


def fixture_cases():
    """[(w, h, [(luma, cb, cr, {sub: outputs})])]: the pictures of every case with the reference's outputs"""
    if "cases" in _cache:
        return _cache["cases"]
    z = fixture()
    out = []
    for c, (w, h) in enumerate(z["case"]):
        pics = []
        for i in range(int(z[f"c{c}_n"])):
            planes = [z[f"c{c}_p{i}_{k}"] for k in ("luma", "cb", "cr")]
            outs = {sub: {k: z[f"c{c}_p{i}_s{sub}_{k}"] for k in OUTPUTS if f"c{c}_p{i}_s{sub}_{k}" in z} for sub in (0, 1)}
            pics.append((*planes, outs))
        out.append((int(w), int(h), pics))
    _cache["cases"] = out
    return out
