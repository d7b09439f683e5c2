"""TEST INFRASTRUCTURE: a numpy restatement of mode decision's interpolation-filter search as svthip_md_model_rd_batch_dev and
svthip_md_interp_filter_search_batch_dev compute it (include/svtav1_hip.h), the constructed cases the CPU and GPU tests share, and the
fixture tests/golden/md_ifs.npz (written by tests/golden/make_golden_md_ifs.py, which asserts this restatement equal to the reference's
own highbd_variance64, av1_model_rd_from_var_lapndz, model_rd_from_sse and interpolation_filter_search).  The trials are predicted by
tests/inter_pred_util.py.

Reference (Source/Lib/Codec/EbInterPrediction.c): interpolation_filter_search :3523-3854, model_rd_for_sb :3378-3468, model_rd_from_sse
:3339-3376, av1_model_rd_from_var_lapndz :3314-3337, model_rd_norm :3248-3312, RDCOST :3241-3244, highbd_8_variance :3161-3190."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import inter_pred_util as ipu  # noqa: E402
import md_fast_util as mfu  # noqa: E402
from abi_util import svtav1_hip  # noqa: E402
from gen_model_rd_tables import DIST, RATE, XSQ  # noqa: E402
from md_fast_util import _texture  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "md_ifs.npz")

# the 17 AV1 block sizes with both sides above 4, (width, height), and their BlockSize values in the reference's enum
SIZES = tuple(s for s in mfu.SIZES if min(s) > 4)
BSIZE = {(8, 8): 3, (8, 16): 4, (16, 8): 5, (16, 16): 6, (16, 32): 7, (32, 16): 8, (32, 32): 9, (32, 64): 10, (64, 32): 11, (64, 64): 12,
         (64, 128): 13, (128, 64): 14, (128, 128): 15, (8, 32): 18, (32, 8): 19, (16, 64): 20, (64, 16): 21}
SEARCH_SIZES = ((8, 8), (16, 8), (8, 16), (32, 32), (64, 64))
MODES = (("fast", 1, 1), ("full", 2, 1), ("no_dual", 2, 0))   # (name, search_mode, enable_dual_filter)
QUANTIZERS = (4, 8, 260, 1828)   # quantizer >> 3 == 0; the smallest step; a middle value; ac_qlookup_Q3[255], the largest of the 8-bit table
REFUSED = 0xFF
MAX_XSQ_Q10 = 245727

# the layouts are the package's, which reads them from include/svtav1_hip.h
MODEL_DESC_DTYPE, MODEL_RESULT_DTYPE, IFS_DESC_DTYPE, IFS_RESULT_DTYPE = (svtav1_hip.md_model_rd_desc_dtype(), svtav1_hip.md_model_rd_result_dtype(),
                                                                          svtav1_hip.md_ifs_desc_dtype(), svtav1_hip.md_ifs_result_dtype())


def _i32(v):
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _i64(v):
    return ((int(v) + (1 << 63)) & 0xFFFFFFFFFFFFFFFF) - (1 << 63)


# ------------------------------------------------------------------------------------------------ the model

def sse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def model_rd_norm(xsq_q10):
    """model_rd_norm: (r_q10, d_q10), linear between the knots of the tables"""
    tmp = (xsq_q10 >> 2) + 8
    k = tmp.bit_length() - 1 - 3
    xq = (k << 3) + ((tmp >> k) & 7)
    a = ((xsq_q10 - XSQ[xq]) << 10) >> (2 + k)
    b = 1024 - a
    return (RATE[xq] * b + RATE[xq + 1] * a) >> 10, (DIST[xq] * b + DIST[xq + 1] * a) >> 10


def model_rd_from_var_lapndz(var, n_log2, qstep):
    """av1_model_rd_from_var_lapndz: (rate, dist)"""
    if var == 0:
        return 0, 0
    xsq = min((((qstep * qstep) << (n_log2 + 10)) + (var >> 1)) // var, MAX_XSQ_Q10)
    r_q10, d_q10 = model_rd_norm(xsq)
    return ((r_q10 << n_log2) + 1) >> 1, (var * d_q10 + 512) >> 10


def qstep_of(quantizer):
    """quantizer >> dequant_shift handed to a uint32_t parameter"""
    return (int(quantizer) >> 3) & 0xFFFFFFFF


def model_rd_from_sse(n_log2, quantizer, sse_):
    rate, dist = model_rd_from_var_lapndz(int(sse_), n_log2, qstep_of(quantizer))
    return rate, dist << 4


def rdcost(lambda_, rate, dist):
    """RDCOST(RM, R, D) with R a 32-bit signed sum: ROUND_POWER_OF_TWO((uint64_t)R * RM, 9) + D * 128, as int64_t"""
    r = _i32(rate) & 0xFFFFFFFFFFFFFFFF
    m = 0xFFFFFFFFFFFFFFFF
    return _i64((((((r * int(lambda_)) & m) + 256) & m) >> 9) + (int(dist) << 7))


def log2(v):
    return int(v).bit_length() - 1


def tile_sses(src, pred, d, w, h):
    """(sse Y, Cb, Cr) of one descriptor; src and pred are (Y, Cb, Cr) arrays; chroma at position / 2"""
    sx, sy, px, py = (int(d[k]) for k in ("src_x", "src_y", "pred_x", "pred_y"))
    out = [sse(src[0][sy:sy + h, sx:sx + w], pred[0][py:py + h, px:px + w])]
    for k in (1, 2):
        a, b = src[k][sy // 2:sy // 2 + h // 2, sx // 2:sx // 2 + w // 2], pred[k][py // 2:py // 2 + h // 2, px // 2:px // 2 + w // 2]
        assert a.shape == b.shape == (h // 2, w // 2), (k, d)
        out.append(sse(a, b))
    return out


def model_result(sses, lambda_, rate, w, h, quantizer):
    """MODEL_RESULT_DTYPE scalar from the three SSEs: model_rd_for_sb's sums and the RDCOST on top"""
    n = log2(w * h)
    parts = [model_rd_from_sse(n if k == 0 else n - 2, quantizer, s) for k, s in enumerate(sses)]
    r = np.zeros((), MODEL_RESULT_DTYPE)
    r["sse"] = sses
    r["rate"] = _i32(sum(p[0] for p in parts))
    r["dist"] = sum(p[1] for p in parts)
    r["rd"] = rdcost(lambda_, _i32(int(rate) + int(r["rate"])), int(r["dist"]))
    return r


def model_rd(src, pred, desc, w, h, quantizer):
    """svthip_md_model_rd_batch_dev: (MODEL_RESULT_DTYPE[n], number refused); a descriptor with an odd position gives a zero row"""
    out, refused = np.zeros(len(desc), MODEL_RESULT_DTYPE), 0
    for i, d in enumerate(desc):
        if (int(d["src_x"]) | int(d["src_y"]) | int(d["pred_x"]) | int(d["pred_y"])) & 1:
            refused += 1
            continue
        out[i] = model_result(tile_sses(src, pred, d, w, h), d["lambda_"], d["rate"], w, h, quantizer)
    return out, refused


# ------------------------------------------------------------------------------------------------ the search

def trial_filters(t):
    """av1_make_interp_filters(filter_sets[t][0], filter_sets[t][1]): y filter t // 3 low, x filter t % 3 high"""
    return (t // 3) | ((t % 3) << 16)


def trial_rate(f, t):
    return _i32(int(f["filter_rate"][0][t // 3]) + int(f["filter_rate"][1][t % 3]))


def walk(search_mode, dual, measure):
    """The compares of interpolation_filter_search.  measure(trial) -> (rd, total_sse, rs).  Returns (best trial, rd, rs, total_sse of the
    best, the trials measured in order)."""
    seen = [0]
    rd, total, rs = measure(0)
    best = 0

    def visit(i):
        nonlocal rd, total, rs, best
        seen.append(i)
        t_rd, t_total, t_rs = measure(i)
        if t_rd < rd:
            rd, total, rs, best = t_rd, t_total, t_rs, i
            return True
        return False

    if search_mode == 1 and dual:
        best_dual_mode = 0
        for i in (1, 2):
            # :3630-3631 store (InterpFilter)av1_make_interp_filters(..): InterpFilter is a one-byte enum in a GCC / Clang build, the x filter
            # in bits 16.. is cut off, and what is predicted and priced is the trial of the y filter alone -- trial 0 again, never < rd
            if visit(3 * (trial_filters(i) & 0xFF)):
                best_dual_mode = i
        for i in (best_dual_mode + 3, best_dual_mode + 6):
            visit(i)
    else:
        for i in range(1, 9):
            if not dual and i // 3 != i % 3:
                continue
            visit(i)
    return best, rd, rs, total, seen


class Trials:
    """the nine trial measurements of one candidate, each made once: tile prediction by inter_pred_util, then the model"""

    def __init__(self, ref0, ref1, src, pu, f, w, h, quantizer):
        self.args, self.cache, self.tiles = (ref0, ref1, src, pu, f, w, h, quantizer), {}, {}

    def tile(self, t):
        ref0, ref1, src, pu, f, w, h, quantizer = self.args
        if t not in self.tiles:
            d = pu.copy()
            d["interp_filters"], d["dst_origin_x"], d["dst_origin_y"], d["has_uv"] = trial_filters(t), 0, 0, 1
            tile = ipu.Picture(np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8), 0)
            assert ipu.predict_pu(ref0, ref1, tile, d, w, h, 8)
            self.tiles[t] = tile
        return self.tiles[t]

    def __call__(self, t):
        ref0, ref1, src, pu, f, w, h, quantizer = self.args
        if t not in self.cache:
            tile = self.tile(t)
            m = np.zeros((), MODEL_DESC_DTYPE)
            m["src_x"], m["src_y"] = f["src_x"], f["src_y"]
            sses = tile_sses(src, (tile.y, tile.cb, tile.cr), m, w, h)
            r = model_result(sses, f["lambda_"], trial_rate(f, t), w, h, quantizer)
            self.cache[t] = (int(r["rd"]), sum(sses), trial_rate(f, t))
        return self.cache[t]


def search_one(trials, search_mode, dual):
    """IFS_RESULT_DTYPE scalar of one candidate, and the trials it measured"""
    best, rd, rs, total, seen = walk(search_mode, dual, trials)
    r = np.zeros((), IFS_RESULT_DTYPE)
    r["interp_filters"], r["switchable_rate"], r["rd"], r["skip_sse_sb"], r["skip_txfm_sb"], r["best_trial"] = trial_filters(best), rs, rd, total << 4, total == 0, best
    return r, seen


def refused_row():
    r = np.zeros((), IFS_RESULT_DTYPE)
    r["best_trial"] = REFUSED
    return r


def search(cands, search_mode, dual, refused=()):
    """svthip_md_interp_filter_search_batch_dev over a list of Trials: (IFS_RESULT_DTYPE[n], number refused).  A candidate is refused when
    its source position is odd or when the caller says its PU is one the prediction refuses (`refused`: indices)."""
    out, n_refused = np.zeros(len(cands), IFS_RESULT_DTYPE), 0
    for i, c in enumerate(cands):
        f = c.args[4]
        if i in refused or (int(f["src_x"]) | int(f["src_y"])) & 1:
            out[i], n_refused = refused_row(), n_refused + 1
        else:
            out[i] = search_one(c, search_mode, dual)[0]
    return out, n_refused


# ------------------------------------------------------------------------------------------------ constructed cases: the model entry

def model_descriptors(z, n, variant=0):
    """n descriptors of size SIZES[z] over the six tiles of md_fast_util.pool_planes (source positions multiples of 4, tiles at multiples of
    8 ringed by 0 and 255); lambdas up to 32 bits, rates of both signs"""
    w, h = SIZES[z]
    fd = mfu.descriptors(mfu.SIZES.index((w, h)), n, variant)
    d = np.zeros(n, MODEL_DESC_DTYPE)
    for k in ("src_x", "src_y", "pred_x", "pred_y"):
        d[k] = fd[k]
    for i in range(n):
        d[i]["lambda_"] = (97 + 2111 * i + variant) if i % 5 else 0xFFFFFFF1
        d[i]["rate"] = (1000 + 977 * i + 31 * z) * (-1 if i % 7 == 3 else 1)
    return d


def model_planes(z):
    """(source planes, pool planes) of size SIZES[z]"""
    src = mfu.source_planes()
    return src, mfu.pool_planes(mfu.SIZES.index(SIZES[z]), src)


def extreme_tile():
    """one 128 x 128 tile in which every difference is 255: (src planes, pred planes, descriptor)"""
    src = [np.full((128, 128), 255, np.uint8), np.zeros((64, 64), np.uint8), np.full((64, 64), 255, np.uint8)]
    pred = [np.zeros((128, 128), np.uint8), np.full((64, 64), 255, np.uint8), np.zeros((64, 64), np.uint8)]
    d = np.zeros(1, MODEL_DESC_DTYPE)
    d["lambda_"], d["rate"] = 0xFFFFFFFF, 0x7FFFFFF0
    return src, pred, d


# ------------------------------------------------------------------------------------------------ constructed cases: the search

PIC_W, PIC_H, BORDER = 192, 128, 80
SKIP_MV = (32, -48)     # (row, col) in 1/8 luma sample: 4 down, 6 left -- whole samples in chroma too
N_KINDS = 16
FORCE_LAMBDA, FORCE_RATE = 0x7FFFFFFF, 500000000


def _smooth(w, h, seed):
    """a texture with structure at the scale of the filters: the noise of md_fast_util._texture averaged over 3 x 3, contrast restored"""
    t = _texture(w + 2, h + 2, seed).astype(np.int32)
    s = sum(t[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return np.clip((s - 9 * 128) // 3 + 128, 0, 255).astype(np.uint8)


def _picture(seed):
    def plane(pw, ph, b, k):
        return _smooth(pw + 2 * b + 32, ph + 2 * b, seed + k)
    return ipu.Picture(plane(PIC_W, PIC_H, BORDER, 0), plane(PIC_W // 2, PIC_H // 2, BORDER // 2, 1), plane(PIC_W // 2, PIC_H // 2, BORDER // 2, 2), BORDER)


_PICTURES = None


def search_pictures():
    """(ref0, ref1, src): two padded reference pictures and the source planes (Y, Cb, Cr at sample (0, 0), no padding).  The source is
    reference 0 moved by (1.5, 2.5) luma samples plus a little noise, so that the filters matter and no one always wins; its top-left 64 x 64
    is reference 0 moved by SKIP_MV exactly (the candidate every filter predicts without error)."""
    global _PICTURES
    if _PICTURES is None:
        ref0, ref1 = _picture(300), _picture(310)
        src = []
        for k, (p, b) in enumerate(((ref0.y, BORDER), (ref0.cb, BORDER // 2), (ref0.cr, BORDER // 2))):
            ph, pw = (PIC_H, PIC_W) if k == 0 else (PIC_H // 2, PIC_W // 2)
            q = p.astype(np.int32)
            oy, ox = (1, 2) if k == 0 else (0, 1)
            a = sum(q[b + oy + dy:b + oy + dy + ph, b + ox + dx:b + ox + dx + pw] for dy in (0, 1) for dx in (0, 1))
            s = np.clip((a + 2) // 4 + (_texture(pw, ph, 320 + k).astype(np.int32) - 128) // 16, 0, 255).astype(np.uint8)
            n, my, mx = (64, SKIP_MV[0] // 8, SKIP_MV[1] // 8) if k == 0 else (32, SKIP_MV[0] // 16, SKIP_MV[1] // 16)
            s[:n, :n] = p[b + my:b + my + n, b + mx:b + mx + n]
            src.append(s)
        _PICTURES = (ref0, ref1, tuple(src))
    return _PICTURES


def _hash(*v):
    x = 0x9E3779B9
    for k in v:
        x = ((x ^ (int(k) & 0xFFFFFFFF)) * 0x85EBCA6B + 0xC2B2AE35) & 0xFFFFFFFF
        x ^= x >> 15
    return x


def search_cases(size, n, variant=0):
    """n candidates of one size: (INTER_PU_DESC_DTYPE[n], IFS_DESC_DTYPE[n]).  Candidate k is of kind k % 16:
      0..8   the rates make trial `kind` win in every mode that reaches it (the full mode reaches all nine, the fast mode 0, 3 and 6,
             the mode without the dual filter 0, 4 and 8): filter_rate 0 for its two filters, FORCE_RATE for the others, a lambda that
             lets the rate decide
      9      whole-sample vectors (every trial predicts the same) and all rates 0: nine exact ties, trial 0 stays under `<`
      10     whole-sample vectors, rates 50 / 0 / 0 both ways: trials 4, 5, 7, 8 tie below the others; the first one met wins
      11     list 0, SKIP_MV, the block at (0, 0): every prediction equals the source, all rates 0: skip_txfm_sb = 1, rd = 0
      12..15 small rates and a moderate lambda: the distortion decides
    Directions cycle 0, 1, 2 (uni list 0, uni list 1, bi); positions and vectors wander with k and the variant."""
    import svtav1_hip
    w, h = size
    pu, f = np.zeros(n, svtav1_hip.INTER_PU_DESC_DTYPE), np.zeros(n, IFS_DESC_DTYPE)
    cols, rows = PIC_W // w, PIC_H // h
    for k in range(n):
        kind, r = k % N_KINDS, _hash(w, h, k, variant)
        slot = (k * 7 + variant) % (cols * rows)
        x, y = (slot % cols) * w, (slot // cols) * h
        direction = (k // N_KINDS + k + variant) % 3
        whole = kind in (9, 10)   # vectors of whole samples in luma and chroma (multiples of 16), else anything within 8 samples
        mv = [[(((r >> (8 * l + 4 * c)) & 7) - 4) * 16 if whole else ((r >> (8 * l + 4 * c)) & 0x7F) - 64 for c in range(2)] for l in range(2)]
        if kind == 11:
            x, y, direction, mv = 0, 0, 0, [list(SKIP_MV), [0, 0]]
        pu[k]["pu_origin_x"], pu[k]["pu_origin_y"] = x, y
        pu[k]["dst_origin_x"], pu[k]["dst_origin_y"] = 0xFFF8, 0xFFF8          # ignored on input
        pu[k]["interp_filters"] = 0x00030003                                    # ignored on input
        pu[k]["mb_to_left_edge"], pu[k]["mb_to_right_edge"] = -x * 8, (PIC_W - w - x) * 8
        pu[k]["mb_to_top_edge"], pu[k]["mb_to_bottom_edge"] = -y * 8, (PIC_H - h - y) * 8
        pu[k]["pred_direction"], pu[k]["has_uv"], pu[k]["own_list"] = direction, 1, int(direction == 1)
        pu[k]["mv"] = mv
        f[k]["src_x"], f[k]["src_y"] = x, y
        if kind < 9:
            f[k]["lambda_"] = FORCE_LAMBDA
            f[k]["filter_rate"] = [[0 if j == kind // 3 else FORCE_RATE + 13 * j for j in range(3)], [0 if j == kind % 3 else FORCE_RATE + 7 * j for j in range(3)]]
        elif kind == 10:
            f[k]["lambda_"], f[k]["filter_rate"] = 40000 + k, [[50, 0, 0], [50, 0, 0]]
        elif kind in (9, 11):
            f[k]["lambda_"], f[k]["filter_rate"] = 40000 + k, 0
        else:
            f[k]["lambda_"] = 3000 + (r >> 20)
            f[k]["filter_rate"] = [[30 + (r >> (3 * j)) % 400 for j in range(3)], [20 + (r >> (5 * j + 1)) % 500 for j in range(3)]]
    return pu, f


def search_trials(size, n, quantizer, variant=0):
    """(pu, ifs, [Trials]) of search_cases"""
    ref0, ref1, src = search_pictures()
    pu, f = search_cases(size, n, variant)
    return pu, f, [Trials(ref0, ref1, src, pu[k], f[k], size[0], size[1], quantizer) for k in range(n)]


def search_quantizer(size):
    """one quantizer per size of the fixture's search cases"""
    return {(8, 8): 260, (16, 8): 64, (8, 16): 1828, (32, 32): 420, (64, 64): 36}[tuple(size)]


_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(FIXTURE) as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE
