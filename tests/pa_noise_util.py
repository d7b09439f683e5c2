"""TEST INFRASTRUCTURE ONLY -- input-picture noise detection and denoising of include/svtav1_hip.h (svthip_pa_noise_detect_dev,
svthip_pa_denoise_dev) restated with numpy integers from the reference's FullSampleDenoise (Codec/EbPictureAnalysisProcess.c:3357-3410):
noiseExtractLumaWeak (:1501-1561) with getFilteredTypes type 0 (:1207-1213), ComputeVariance64x64 (:360-1197) of the noise and of the
denoised luma, the class ladder of DetectInputPictureNoise (:3181-3320), noiseExtractChromaWeak (:1414-1495, type 4) and the three arms of
DenoiseInputPicture (:3007-3179).  Takes the unpadded planes of a picture and never looks outside them.
tests/golden/make_golden_pa_noise.py asserts it equal to the reference while it writes tests/golden/pa_noise.npz;
tests/test_pa_noise_vs_ref.py, tests/test_pa_noise_kernels_host.py and tests/test_pa_noise_gpu.py compare against it and the fixture."""
import os

import numpy as np

import pa_stats_util as pu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "pa_noise.npz")
# width, height; every case at both precisions
CASES = ((64, 64), (136, 72), (72, 136), (192, 192), (200, 136), (136, 728))
DETECT_OUTPUTS = ("sb_var", "flat_noise", "picture")
U64 = np.uint64
FLAT_MAX_VAR, NOISE_MIN_LEVEL_M6_M7 = 50, 120000
CLASS_1, CLASS_2, CLASS_3, CLASS_3_1, CLASS_4 = 1, 2, 3, 4, 5          # EbDefinitions.h:2753-2764; PIC_NOISE_CLASS_10 is 11
LADDER = ((80, 11), (70, 10), (60, 9), (50, 8), (40, 7), (30, 6), (20, 5), (17, 4), (10, 3), (5, 2))
ARMS = ("whole_picture", "flat_sbs", "nothing")


def weak_luma(luma):
    """-> (denoised, noise), both uint8 [h][w]: the outermost rows and columns are copied and carry no noise"""
    p = luma.astype(np.int32)
    den, noise = p.copy(), np.zeros_like(p)
    c = p[1:-1, 1:-1]
    d = (p[:-2, 1:-1] + p[1:-1, :-2] + 4 * c + p[1:-1, 2:] + p[2:, 1:-1]) // 8
    den[1:-1, 1:-1] = d
    noise[1:-1, 1:-1] = np.maximum(c - d, 0)
    return den.astype(np.uint8), noise.astype(np.uint8)


def weak_chroma(plane):
    """the 1 2 1 / 2 4 2 / 1 2 1 kernel / 16 inside, the outermost rows and columns copied"""
    p = plane.astype(np.int32)
    out = p.copy()
    out[1:-1, 1:-1] = (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:] + 2 * p[1:-1, :-2] + 4 * p[1:-1, 1:-1] + 2 * p[1:-1, 2:] + p[2:, :-2] + 2 * p[2:, 1:-1] +
                       p[2:, 2:]) // 16
    return out.astype(np.uint8)


def variance64(plane, sub):
    """ComputeVariance64x64 of every SB of a plane: raw 16.16 in uint64, [n_sb] in raster order (incomplete SBs from replicated samples: unused)"""
    h, w = plane.shape
    nx, ny = pu.sb_grid(w, h)
    m, s = pu._leaf_tables(plane, nx, ny, int(bool(sub)))
    for _ in range(3):
        m, s = pu._up(m), pu._up(s)
    return (s - m * m).reshape(-1)


def noise_class(avg, height):
    """-> (class as the reference leaves it, class before the clamp of :3315)"""
    th = 25 if height <= 720 else 0
    raw = next((c for t, c in LADDER if avg >= t + th), CLASS_1)
    return (CLASS_3_1 if raw >= CLASS_4 else raw), raw


def detect(luma, sub):
    """-> {"sb_var": [n_sb][2] u64 (noise_var raw, den_var >> 16), "flat_noise": [n_sb] u8, "picture": [4] u32 = sum, count, class, sum >= count,
    "denoised": [h][w] u8, "noise": [h][w] u8, "raw_class": int}"""
    h, w = luma.shape
    den, noise = weak_luma(luma)
    complete = pu.complete_sbs(w, h)
    assert complete.any(), "no complete SB: the reference divides by zero"
    nv, dv = variance64(noise, sub), variance64(den, sub) >> U64(16)
    sb_var = np.stack([nv, dv], 1)
    sb_var[~complete] = 0
    flat = (complete & (dv < FLAT_MAX_VAR) & (nv > NOISE_MIN_LEVEL_M6_M7)).astype(np.uint8)
    total, count = int((nv[complete] >> U64(16)).sum()), int(complete.sum())
    cls, raw = noise_class(total // count, h)
    return {"sb_var": sb_var, "flat_noise": flat, "picture": np.array([total, count, cls, total >= count], np.uint32), "denoised": den, "noise": noise,
            "raw_class": raw}


def arm(picture):
    return ARMS[0] if picture[2] >= CLASS_3_1 else ARMS[1] if picture[3] else ARMS[2]


def denoise(luma, cb, cr, det):
    """the input picture after DenoiseInputPicture -> (luma, cb, cr)"""
    whole = arm(det["picture"]) == "whole_picture"
    return _assemble(luma, cb, cr, det, weak_chroma(cb) if whole else None, weak_chroma(cr) if whole else None)


def _assemble(luma, cb, cr, det, den_cb, den_cr):
    """the planes after DenoiseInputPicture from its pieces: the flags and the class in `det` choose the arm, det["denoised"] and (for the
    whole-picture arm) den_cb / den_cr are the samples.  The fixture stores the reference's pieces and not the planes; the generator asserted
    that the reference's planes are made of them this way"""
    a = arm(det["picture"])
    if a == "whole_picture":
        assert den_cb is not None and den_cr is not None
        return det["denoised"].copy(), den_cb, den_cr
    h, w = luma.shape
    out = luma.copy()
    if a == "flat_sbs":
        nx, _ = pu.sb_grid(w, h)
        for sb in np.flatnonzero(det["flat_noise"]):
            y0, x0 = (sb // nx) * 64, (sb % nx) * 64
            out[y0:y0 + 64, x0:x0 + 64] = det["denoised"][y0:y0 + 64, x0:x0 + 64]
    return out, cb.copy(), cr.copy()


# ---------------------------------------------------------------------------------------------- the fixture

COVERAGE_KEYS = ("flat_0", "flat_1", "incomplete_sb_right", "incomplete_sb_bottom", "centre_sb_with_four_neighbours",
                 "th25_class_1", "th25_class_2", "th25_class_3", "th25_class_3_1", "th0_class_1", "th0_class_2", "th0_class_3", "th0_class_3_1",
                 "th25_clamped", "th0_clamped", "below_3_1_sum_ge_count", "below_3_1_sum_lt_count", "arm_whole_picture", "arm_flat_sbs", "arm_nothing",
                 "flat_sbs_arm_changes_luma", "noise_clips_to_0", "sub_differs_from_full", "chroma_filter_changes_chroma")


def coverage(cases):
    """cases: [(w, h, luma, cb, cr, {sub: reference outputs})] -> {key: reached}; from the reference's outputs alone (and the input planes)"""
    c = dict.fromkeys(COVERAGE_KEYS, False)
    for (w, h, luma, cb, cr, outs) in cases:
        comp = pu.complete_sbs(w, h)
        c["incomplete_sb_right"] |= w % 64 != 0
        c["incomplete_sb_bottom"] |= h % 64 != 0
        c["centre_sb_with_four_neighbours"] |= w >= 192 and h >= 192
        p = luma.astype(np.int32)
        d = outs[0]["denoised"].astype(np.int32)
        c["noise_clips_to_0"] |= bool((p[1:-1, 1:-1] < d[1:-1, 1:-1]).any())
        c["sub_differs_from_full"] |= not np.array_equal(outs[0]["sb_var"], outs[1]["sb_var"])
        for o in outs.values():
            total, count, cls, ge = (int(v) for v in o["picture"])
            th = "th25" if h <= 720 else "th0"
            c["flat_0"] |= bool((o["flat_noise"][comp] == 0).any())
            c["flat_1"] |= bool((o["flat_noise"][comp] == 1).any())
            raw = noise_class(total // count, h)[1]
            if raw >= CLASS_4:
                c[f"{th}_clamped"] = True
            else:
                c[f"{th}_class_{('1', '2', '3', '3_1')[cls - 1]}"] = True
            if cls < CLASS_3_1:
                c["below_3_1_sum_ge_count" if ge else "below_3_1_sum_lt_count"] = True
            a = arm(o["picture"])
            c[f"arm_{a}"] = True
            c["flat_sbs_arm_changes_luma"] |= a == "flat_sbs" and not np.array_equal(o["out_luma"], luma)
            c["chroma_filter_changes_chroma"] |= a == "whole_picture" and not np.array_equal(o["out_cb"], cb)
    return c


_cache = {}
FIXTURE_OUTPUTS = DETECT_OUTPUTS + ("denoised", "out_luma", "out_cb", "out_cr")


def fixture():
    if "z" not in _cache:
        _cache["z"] = dict(np.load(FIXTURE))
    return _cache["z"]


def fixture_cases():
    """[(w, h, [(luma, cb, cr, {sub: outputs})])]: the pictures of every case with what the reference left (FIXTURE_OUTPUTS)"""
    if "cases" in _cache:
        return _cache["cases"]
    z = fixture()
    out = []
    for c, (w, h) in enumerate(z["case"]):
        pics = []
        for i in range(int(z[f"c{c}_n"])):
            luma = z[f"c{c}_p{i}_luma"]
            cb, cr = chroma_of(luma)
            outs = {}
            for sub in (0, 1):
                o = {k: z[f"c{c}_p{i}_s{sub}_{k}"] for k in DETECT_OUTPUTS}
                # the planes are not stored twice: the fixture keeps the reference's denoised luma and chroma once per picture (they do not depend
                # on the precision) and the generator asserted that the planes after DenoiseInputPicture are made of them as `denoise` says
                o["denoised"] = z[f"c{c}_p{i}_denoised"]
                det = dict(o)
                o["out_luma"], o["out_cb"], o["out_cr"] = _assemble(luma, cb, cr, det, z.get(f"c{c}_p{i}_den_cb"), z.get(f"c{c}_p{i}_den_cr"))
                outs[sub] = o
            pics.append((luma, cb, cr, outs))
        out.append((int(w), int(h), pics))
    _cache["cases"] = out
    return out


def chroma_of(luma):
    """the chroma planes every fixture picture carries: constructed from its luma, so the fixture need not store them"""
    return np.ascontiguousarray(luma[::2, ::2]), np.ascontiguousarray(255 - luma[1::2, 1::2])
