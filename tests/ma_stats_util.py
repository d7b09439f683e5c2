"""TEST INFRASTRUCTURE ONLY -- the five motion-analysis entries of include/svtav1_hip.h (svthip_ma_zz_sad_dev, svthip_ma_ac_energy_dev,
svthip_ma_distortion_stats_dev, svthip_ma_global_motion_dev, svthip_ma_sb_flags_dev) restated with numpy and Python integers from the
reference (ComputeDecimatedZzSad, CalculateAcEnergy, the tail of MotionEstimateLcu and the histogram loop of MotionEstimationKernel,
DetectGlobalMotion / MeBasedGlobalMotionDetection, DeriveSimilarCollocatedFlag, FailingMotionLcu, DetectUncoveredLcu).
tests/golden/make_golden_ma_stats.py asserts it equal to the reference's functions while it writes tests/golden/ma_stats.npz.  The
rc_me_distortion sum and the histogram loop are inline in the reference (MotionEstimateLcu, the ME thread's body) and the counters of
DetectGlobalMotion are locals: for those this restatement, read against Codec/EbMotionEstimation.c:7150-7158,
Codec/EbMotionEstimationProcess.c:607-725 and Codec/EbInitialRateControlProcess.c:253-406, is the checker."""
import os

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ma_stats.npz")
CASES = ((64, 64), (136, 72), (200, 136), (256, 256))
# the 24-byte svthip_me_cu_result
ME_DTYPE = np.dtype([("xMvL0", "<i2"), ("yMvL0", "<i2"), ("xMvL1", "<i2"), ("yMvL1", "<i2"), ("distortion", "<u4", (3,)), ("direction", "u1", (3,)),
                     ("totalMeCandidateIndex", "u1")])
SENTINEL = 100000000
SIGNALS = ("slice_is_intra", "temporal_layer_index", "hierarchical_levels", "is_used_as_reference_flag", "intensity_transition_flag")
GLOBAL_MOTION_THRESHOLD = ((2,), (4, 2), (8, 4, 2), (16, 8, 4, 2), (32, 16, 8, 4, 2), (64, 32, 16, 8, 4, 2))


def sb_grid(w, h):
    return (w + 63) // 64, (h + 63) // 64


def n_sbs(w, h):
    return sb_grid(w, h)[0] * sb_grid(w, h)[1]


def sb_origins(w, h):
    nx, ny = sb_grid(w, h)
    return [(64 * x, 64 * y) for y in range(ny) for x in range(nx)]


def complete_sbs(w, h):
    return np.array([x + 64 <= w and y + 64 <= h for x, y in sb_origins(w, h)])


# ---------------------------------------------------------------------------------------------- 1. ZZ SAD

def zz_classes(sad):
    """one complete SB's (zz_cost, non_moving_index)"""
    zz = 0 if sad < 256 else 3 if sad < 512 else 10 if sad < 1024 else 20 if sad < 2048 else 30
    return zz, 0 if sad < 512 else 10 if sad < 1024 else 20 if sad < 2048 else 30


def zz_sad(cur, prev):
    """unpadded luma of the current and the previous picture -> sad [n_sb] u32, zz_cost, non_moving_index [n_sb] u8"""
    h, w = cur.shape
    a, b = cur[::4, ::4].astype(np.int64), prev[::4, ::4].astype(np.int64)   # the 1/16 plane; Decimation2D with step 4 of the full plane
    sad, zz, nm = np.full(n_sbs(w, h), 0xffffffff, np.uint32), np.full(n_sbs(w, h), 255, np.uint8), np.full(n_sbs(w, h), 30, np.uint8)
    for i, (x, y) in enumerate(sb_origins(w, h)):
        if x + 64 <= w and y + 64 <= h:
            s = int(np.abs(a[y >> 2:(y >> 2) + 16, x >> 2:(x >> 2) + 16] - b[y >> 2:(y >> 2) + 16, x >> 2:(x >> 2) + 16]).sum())
            sad[i] = s
            zz[i], nm[i] = zz_classes(s)
    return sad, zz, nm


# ---------------------------------------------------------------------------------------------- 2. AC energy

_H8 = np.array([[1]], np.int64)
for _ in range(3):
    _H8 = np.block([[_H8, _H8], [_H8, -_H8]])


def _energy(block):
    """ComputeNxMSatdSadLCU of a block whose sides are multiples of 8"""
    n = block.shape[0] // 8
    b = block.astype(np.int64).reshape(n, 8, n, 8).transpose(0, 2, 1, 3)
    coef = _H8 @ b @ _H8.T
    assert int(np.abs(coef).max()) <= 64 * 255 < 2 ** 15      # the 16-bit lanes of the reference's leaf never wrap
    satd = ((np.abs(coef).sum((2, 3)) + 2) >> 2).sum()
    dc = np.abs(coef[:, :, 0, 0]).sum()
    return int(satd) - (int(dc) >> 2)


def ac_energy(luma, slice_is_intra, y_mean):
    """-> energy, mean [n_sb][5] u64"""
    h, w = luma.shape
    energy, mean = np.full((n_sbs(w, h), 5), SENTINEL, np.uint64), np.full((n_sbs(w, h), 5), SENTINEL, np.uint64)
    if not slice_is_intra:
        return energy, mean
    for i, (x, y) in enumerate(sb_origins(w, h)):
        if x + 64 <= w and y + 64 <= h:
            sb = luma[y:y + 64, x:x + 64]
            energy[i] = [_energy(sb)] + [_energy(sb[32 * (q >> 1):32 * (q >> 1) + 32, 32 * (q & 1):32 * (q & 1) + 32]) for q in range(4)]
            mean[i] = y_mean[i, :5]
    return energy, mean


# ---------------------------------------------------------------------------------------------- 3. distortion statistics

def ois_distortion(words):
    return np.asarray(words, np.uint32) & np.uint32(0xfffff)


def ois_sum32(cand_sb):
    """cand_sb [85][18] words of one SB -> the four 32x32 candidates' distortions summed"""
    return int(ois_distortion(cand_sb[1:5, 0]).astype(np.int64).sum())


def sad_interval(distortion, inter):
    i = distortion >> 8
    if inter:
        i &= 0xffff
    i = (i >> 2) & 0xffff
    if i > 63:
        i = 63 + ((i - 63) >> 3)
    return min(i, 127)


def distortion_stats(me, cand, w, h, slice_is_intra):
    """me [n_sb][>= 85] ME_DTYPE (None on an intra picture), cand [n_sb][85][18] -> rc_me_distortion, inter_index, intra_index [n_sb] u32,
    histograms [2][128] u32, full_sb_count"""
    n = n_sbs(w, h)
    rc, inter, intra = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    hist, full = np.zeros((2, 128), np.uint32), 0
    for i, complete in enumerate(complete_sbs(w, h)):
        if not slice_is_intra:
            rc[i] = int(me[i]["distortion"][5:21, 0].astype(np.uint64).sum()) & 0xffffffff
        if complete:
            if not slice_is_intra:
                inter[i] = sad_interval(int(rc[i]), True)
                hist[0, inter[i]] += 1
            intra[i] = sad_interval(ois_sum32(cand[i]), False)
            hist[1, intra[i]] += 1
            full += 1
    return rc, inter, intra, hist, np.uint32(full)


# ---------------------------------------------------------------------------------------------- 4. global motion

def get_mv(row):
    """GetMv of one ME entry -> (x, y) or None when it has no UNI_PRED_LIST_0 candidate"""
    for k in range(min(int(row["totalMeCandidateIndex"]), 3)):
        if row["direction"][k] == 0:
            return int(row["xMvL0"]), int(row["yMvL0"])
    return None


def _pan(th, ca, cb, na, nb):
    return cb < 16 and nb < 16 and ca * na > 0 and abs(ca) >= th and abs(na) >= th and abs(ca - na) < 16


def _high(th, ca, na):
    return ca * na > 0 and abs(ca) >= th and abs(na) >= th and abs(ca - na) < 16


def _cdiv(a, b):
    """C's signed division, truncating towards zero, then (int16_t)"""
    q = abs(a) // b
    q = -q if a < 0 else q
    return ((q + 0x8000) & 0xffff) - 0x8000


def global_motion(me, w, h, signals):
    """me [n_sb][>= 1] ME_DTYPE -> [12] i32.  A row without a list-0 candidate counts in word 11 and stands for (0, 0): the reference
    carries an earlier SB's vector there, which the entry does not promise"""
    out = np.zeros(12, np.int32)
    if signals["slice_is_intra"]:
        return out
    nx, _ = sb_grid(w, h)
    th = GLOBAL_MOTION_THRESHOLD[signals["hierarchical_levels"]][signals["temporal_layer_index"]]
    mv = [get_mv(me[i][0]) for i in range(n_sbs(w, h))]
    at = lambda i: mv[i] or (0, 0)  # noqa: E731
    checked = pan = tilt = pan_high = tilt_high = no_l0 = 0
    sums = [0, 0, 0, 0]
    for i, (x, y) in enumerate(sb_origins(w, h)):
        if not (x + 64 <= w and y + 64 <= h):
            continue
        no_l0 += mv[i] is None
        cx, cy = at(i)
        nb = [at(i - 1) if x else (0, 0), at(i - nx) if y else (0, 0), at(i + 1) if x + 128 <= w else (0, 0), at(i + nx) if y + 128 <= h else (0, 0)]
        checked += 1
        if any(_pan(th, cx, cy, a, b) for a, b in nb):
            pan, sums[0], sums[1] = pan + 1, sums[0] + cx, sums[1] + cy
        if any(_pan(th, cy, cx, b, a) for a, b in nb):
            tilt, sums[2], sums[3] = tilt + 1, sums[2] + cx, sums[3] + cy
        pan_high += any(_high(th, cx, a) for a, _ in nb)
        tilt_high += any(_high(th, cy, b) for _, b in nb)
    is_pan, is_tilt = pan * 100 // checked > 75, tilt * 100 // checked > 75
    out[:] = [is_pan, is_tilt, _cdiv(sums[0], pan) if is_pan else 0, _cdiv(sums[1], pan) if is_pan else 0, _cdiv(sums[2], tilt) if is_tilt else 0,
              _cdiv(sums[3], tilt) if is_tilt else 0, checked, pan, tilt, pan_high, tilt_high, no_l0]
    return out


# ---------------------------------------------------------------------------------------------- 5. SB flags

def sad_deviation(me_sad, ois_sad):
    diff = me_sad - ois_sad
    return 0 if ois_sad == 0 or diff < 0 else diff * 100 // ois_sad


def sb_flags(y_mean, variance, ref_mean, ref_var, me, cand, w, h, signals):
    """y_mean, variance [n_sb][85]; ref_mean, ref_var [n_sb] -> flags [n_sb][4] u8"""
    flags = np.zeros((n_sbs(w, h), 4), np.uint8)
    if signals["slice_is_intra"]:
        return flags
    for i, complete in enumerate(complete_sbs(w, h)):
        cm, cv, rm, rv = int(y_mean[i, 0]), int(variance[i, 0]), int(ref_mean[i]), max(int(ref_var[i]), 1)
        if abs(cm - rm) < 10 and (abs(cv * 100 // rv - 100) < 10 or abs(cv - rv) < 10):
            flags[i, 0], flags[i, 1] = bool(signals["is_used_as_reference_flag"]), 1
        if not complete or flags[i, 0]:
            continue
        ois = [ois_sum32(cand[i])] + [int(ois_distortion(cand[i, cu, 0])) for cu in range(1, 5)]
        dev = [sad_deviation(int(me[i][cu]["distortion"][0]), ois[cu]) for cu in range(5)]
        quiet = not signals["intensity_transition_flag"]
        flags[i, 2] = any(d > 15 for d in dev) and quiet
        if signals["temporal_layer_index"] == 0:
            flags[i, 3] = any(d > 20 for d in dev) and quiet
    return flags


# ---------------------------------------------------------------------------------------------- the fixture

def signals_dict(values):
    return dict(zip(SIGNALS, (int(v) for v in values)))


_cache = {}


def fixture():
    if "z" not in _cache:
        _cache["z"] = dict(np.load(FIXTURE))
    return _cache["z"]


ZZ_KEYS = ("cur", "prev", "sad", "zz_cost", "non_moving_index")
ENERGY_KEYS = ("luma", "intra", "y_mean", "energy", "mean")
TABLE_KEYS = ("me", "cand", "y_mean", "variance", "ref_mean", "ref_var", "signals", "global_motion", "flags", "compare_global_motion")


def fixture_cases():
    """[(w, h, {"zz": [items], "energy": [items], "tables": [items]})], every item a dict of the inputs and of what the reference left"""
    if "cases" in _cache:
        return _cache["cases"]
    z = fixture()
    out = []
    for c, (w, h) in enumerate(z["case"]):
        groups = {}
        for g, keys in (("zz", ZZ_KEYS), ("energy", ENERGY_KEYS), ("tables", TABLE_KEYS)):
            groups[g] = [{k: z[f"c{c}_{g}{i}_{k}"] for k in keys} for i in range(int(z[f"c{c}_{g}_n"]))]
            for item in groups[g]:
                if "me" in item:
                    item["me"] = item["me"].view(ME_DTYPE).reshape(-1, 85)
        out.append((int(w), int(h), groups))
    _cache["cases"] = out
    return out


def all_tables(item, w, h):
    """the three table entries' outputs for one fixture item, from the restatement"""
    s = signals_dict(item["signals"])
    rc, inter, intra, hist, full = distortion_stats(item["me"], item["cand"], w, h, s["slice_is_intra"])
    return {"rc_me_distortion": rc, "inter_index": inter, "intra_index": intra, "histograms": hist, "full_sb_count": full,
            "global_motion": global_motion(item["me"], w, h, s),
            "flags": sb_flags(item["y_mean"], item["variance"], item["ref_mean"], item["ref_var"], item["me"], item["cand"], w, h, s)}


# ---------------------------------------------------------------------------------------------- the chain test's pictures

def pan_pair(w=256, h=256, shift=5, seed=11):
    """(cur, ref): two windows `shift` samples apart of one texture, blocks of 8 x 8 with noise on top -- a global pan of 4 * shift quarter samples"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(40, 216, ((h + 7) // 8, (w + shift + 7) // 8))
    base = np.kron(coarse, np.ones((8, 8), np.int64))[:h, :w + shift] + rng.integers(-12, 13, (h, w + shift))
    base = np.clip(base, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(base[:, :w]), np.ascontiguousarray(base[:, shift:])
