"""Mode decision as one run of the restatements, for tests/test_md_chain_vs_ref.py, tests/test_md_chain_gpu.py and
tests/golden/make_golden_md_chain.py.  TEST INFRASTRUCTURE: numpy and the oracle only, no reference code.

  interpolation-filter search (filters written back into the PU descriptors) -> inter prediction of every PU into the pool -> intra
  prediction (Y, Cb, Cr) into the same pool -> fast cost -> pick -> full loop LUMA -> the CfL service on the luma the LUMA stage
  reconstructed (alpha candidates -> fused chain and coefficient rate on the 66 tiles a block -> alpha decision -> CfL prediction in place
  over the pool's DC tiles, chroma_rate of those rows changed) -> full loop CHROMA | DECIDE

Every stage is the restatement of its own util (md_ifs_util, inter_pred_util, intra_pred_util, md_fast_util, md_full_util, cfl_util, the
oracle's fused chain and rate_util), each pinned to the reference alone; here each is fed what the stage before it left.  Nothing is
restated again: this file builds the inputs, the descriptors that carry one stage's result into the next, and the two look-ups the header
leaves to the host (which row a slot holds, from the picks; the rate of the chosen alpha).

One scenario per luma size (SIZES) on a 128 x 64 8-bit 4:2:0 source picture: two padded reference pictures, one neighbour picture the
intra edges are read from, blocks at the four picture corners and along every edge, 3 to 7 candidates a block.  Everything is regenerated
from seeds; tests/golden/md_chain.npz holds digests of the inputs and what the chain made of them."""
import contextlib
import hashlib
import os

import numpy as np

import cfl_util as cu
import inter_pred_util as ipu
import intra_pred_util as iu
import md_fast_util as mu
import md_full_util as fu
import md_ifs_util as su
import rate_util
import svtav1_hip
import tq_util

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "md_chain.npz")
PIC_W, PIC_H = 128, 64
MAX_FULL, BUFFER_WIDTH = 4, 13
QUANTIZER = 260                       # the filter search's model quantizer
POOL_FILL = 0x11
EXACT_MV = (16, -16)                  # (row, col) in 1/8 luma sample, whole samples in chroma too: the merge candidates' vector
CFL_MODE_BITS, DC_MODE_BITS = 300, 400
NONE = fu.NONE
# name -> luma size, number of blocks, filter search (None, "fast", "full"), CfL, tx-type search, the refusal scenario
SIZES = {"4x16": ((4, 16), 16, None, False, "m1", False),
         "8x8": ((8, 8), 14, "fast", True, "m1", False),
         "16x16": ((16, 16), 12, "full", True, "m0", False),
         "32x8": ((32, 8), 12, "fast", True, "none", False),
         "64x64": ((64, 64), 2, "fast", False, "m0", False),
         "4x16_refusals": ((4, 16), 12, None, False, "m1", True)}
CHAIN_SIZES = tuple(n for n in SIZES if not SIZES[n][5])
# candidate kinds: inter by list and vector (f fractional, w whole samples), a merge candidate (no filter search), intra by luma mode
KINDS = ("DC", "L0f", "V", "BI", "PAETH", "L1f", "SMOOTH", "L0w", "DIR", "H", "MERGE", "L1w", "BIw")
# the candidates of a size with two blocks: intra ones and the exact merge candidate, made dear, in the first; searched ones in the second
TWO_GROUPS = (("DC", "MERGE", "PAETH", "SMOOTH", "DIR", "V", "H"), ("L0f", "DC", "L1f", "BI"))
INTRA_MODE = {"DC": (iu.DC, 0), "V": (iu.V, 0), "H": (iu.H, 0), "PAETH": (iu.PAETH, 0), "SMOOTH": (iu.SMOOTH, 0)}
DIRECTIONAL = ((iu.D135, 2), (iu.D67, -1), (iu.D45, 3), (iu.D157, -2))
# the arrays and plane sets of the chain, in chain order
STAGES = ("ifs", "pu", "pool_luma", "fast", "picks", "slot_luma", "cfl", "pool_chroma", "result", "decision", "recon")
PLANE_STAGES = ("pool_luma", "slot_luma", "pool_chroma", "recon")


class Scenario:
    """one size's inputs; the fields md_full_util.full_loop reads (w, h, src, pool, fast, full, groups, picks, ...) and the chain's own"""


# ---------------------------------------------------------------- pictures

def _field(w, h, ox, oy, k, shift=(0.0, 0.0)):
    """a smooth picture of plane k (0 Y, 1 Cb, 2 Cr) sampled at picture position (x - ox, y - oy) + shift, in luma units; in the left half
    the chroma planes follow the luma's detail with opposite signs, which is what chroma-from-luma finds, in the right half they do not"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    s = 1 + (k > 0)
    x, y = (xx - ox) * s + shift[0], (yy - oy) * s + shift[1]
    luma = 55 * np.sin(x / 9.0) * np.cos(y / 7.0) + 30 * np.sin((x + 2 * y) / 4.3)
    if k == 0:
        return 128 + luma
    return 128 + (0.45, -0.35)[k - 1] * luma * (x < PIC_W // 2) + (18 + 30 * (x >= PIC_W // 2)) * np.sin(x / 23.0 + k) * np.cos(y / 17.0)


def _picture(rng, border, shift, noise):
    def plane(k):
        b = border >> (k > 0)
        w, h = (PIC_W >> (k > 0)) + 2 * b + 32, (PIC_H >> (k > 0)) + 2 * b
        return np.clip(_field(w, h, b, b, k, shift) + rng.normal(0, noise, (h, w)), 0, 255).astype(np.uint8)
    return ipu.Picture(plane(0), plane(1), plane(2), border)


def _pictures(rng, w, h):
    """(ref0, ref1, source planes, neighbour planes): the source is the field half a luma sample right of and below reference 0, so that
    the vectors near (4, 4) predict it well and the filters matter; its top-left 64 x 64 is reference 0 moved by EXACT_MV exactly (a
    prediction without residual: eob 0)"""
    border = ipu.border_for(w, h)
    ref0, ref1 = _picture(rng, border, (0.0, 0.0), 3), _picture(rng, border, (1.75, -1.25), 4)
    src = [np.clip(_field(PIC_W >> (k > 0), PIC_H >> (k > 0), 0, 0, k, (0.5, 0.5)) + rng.normal(0, 2, (PIC_H >> (k > 0), PIC_W >> (k > 0))), 0, 255).astype(np.uint8)
           for k in range(3)]
    for k, (p, b) in enumerate(((ref0.y, border), (ref0.cb, border // 2), (ref0.cr, border // 2))):     # the top-left quarter: reference 0 moved by EXACT_MV
        n, my, mx = 64 >> (k > 0), EXACT_MV[0] >> (3 + (k > 0)), EXACT_MV[1] >> (3 + (k > 0))
        src[k][:n, :n] = p[b + my:b + my + n, b + mx:b + mx + n]
    nb = [np.clip(p.astype(np.int32) + rng.integers(-5, 6, p.shape), 0, 255).astype(np.uint8) for p in src]
    return ref0, ref1, src, nb


def block_positions(w, h, n):
    """n distinct blocks of the w x h grid: the four corners, then blocks of both edge rows and columns, then the inside"""
    cols, rows = PIC_W // w, PIC_H // h
    cells = [(0, 0), (cols - 1, 0), (0, rows - 1), (cols - 1, rows - 1)]
    edge = [(c, r) for r in range(rows) for c in range(cols) if (c in (0, cols - 1) or r in (0, rows - 1)) and (c, r) not in cells]
    inside = [(c, r) for r in range(1, rows - 1) for c in range(1, cols - 1)]
    k = 0
    while len(cells) < n and (edge or inside):
        take = edge if edge and (k % 3 != 2 or not inside) else inside
        cells.append(take.pop((7 * k + 3) % len(take)))
        k += 1
    cells = list(dict.fromkeys(cells))[:n]
    return [(c * w, r * h) for c, r in cells]


# ---------------------------------------------------------------- the scenario

def make_scenario(name):
    """the inputs of size `name`, from its seed; a new object every time (the chain changes pool, pu, picks and full)"""
    (w, h), n_groups, ifs, cfl, search, refusals = SIZES[name]
    rng = np.random.default_rng(sum(name.encode()) * 13 + 5)
    s = Scenario()
    s.name, s.w, s.h, s.ifs, s.cfl, s.refusals = name, w, h, ifs, cfl, refusals
    s.cw, s.ch = fu.chroma_size(w, h)
    s.ts_y, s.ts_uv = fu.tx_size_of(w, h), fu.tx_size_of(s.cw, s.ch)
    s.max_full, s.reduced = MAX_FULL, 0
    s.mask_inter, s.mask_intra = fu.masks_of(w, h, search, 0)
    s.tw, s.th = max(8, w), max(8, h)
    s.ref0, s.ref1, s.src, s.nb = _pictures(rng, w, h)
    s.block_xy = block_positions(w, h, n_groups)
    s.n_groups = n_groups = len(s.block_xy)

    counts = rng.integers(3, 8, n_groups)
    if n_groups < 3:
        counts[:] = 7
    invalid_groups = [g for g in range(n_groups) if g % 6 == 2 or (n_groups < 3 and g == 1)]
    totals = np.array([1 + (3 * g + 1) % 4 for g in range(n_groups)])
    for g in invalid_groups:                      # every candidate of the group reaches the full loop, the INVALID one (the last: the walk keeps it) too
        counts[g], totals[g] = min(counts[g], 4), 4
    s.n_cand = n_cand = int(counts.sum())
    fast, full, groups = np.zeros(n_cand, fu.FAST_DTYPE), np.zeros(n_cand, fu.FULL_DTYPE), np.zeros(n_groups, fu.GROUP_DTYPE)
    s.kind, s.luma_mode, s.uv_mode = [], np.zeros((n_cand, 2), np.int32), np.zeros((n_cand, 2), np.int32)
    pool_rows = (n_cand + fu.POOL_TILES_PER_ROW - 1) // fu.POOL_TILES_PER_ROW
    s.pool = [np.full((pool_rows * s.th, fu.POOL_TILES_PER_ROW * s.tw), POOL_FILL, np.uint8)] + \
             [np.full((pool_rows * s.th // 2, fu.POOL_TILES_PER_ROW * s.tw // 2), POOL_FILL, np.uint8) for _ in range(2)]
    types_y, types_uv = svtav1_hip.valid_tx_types(w, h), svtav1_hip.valid_tx_types(s.cw, s.ch)
    pus = []
    row = 0
    for g, (x, y) in enumerate(s.block_xy):
        has_uv = ipu.geometry_has_uv(w, h, x, y)
        groups[g] = (row, counts[g], totals[g], BUFFER_WIDTH)
        for j in range(int(counts[g])):
            kind = "DC" if cfl and j == 0 and g % 2 == 0 else "MERGE" if g == 0 and j == 1 else TWO_GROUPS[g][j] if n_groups < 3 else KINDS[(3 * g + 2 * j + (j > 5)) % len(KINDS)]
            px, py = (row % fu.POOL_TILES_PER_ROW) * s.tw, (row // fu.POOL_TILES_PER_ROW) * s.th
            inter = kind not in INTRA_MODE and kind != "DIR"
            f, d = fast[row], full[row]
            f["src_x"], f["src_y"], f["pred_x"], f["pred_y"], f["has_uv"] = x, y, px, py, has_uv
            f["flags"] = (mu.TYPE_INTER if inter else 0) | (mu.INVALID if g in invalid_groups and j == counts[g] - 1 else 0)
            f["rate"], f["merge_rate"], f["lambda_"] = rng.integers(100, 6000), mu.NO_MERGE, rng.integers(300, 2500)
            d["luma_rate"], d["chroma_rate"], d["skip_mode_rate"] = rng.integers(50, 3000), rng.integers(10, 900), NONE
            d["lambda_"] = rng.integers(2000, 60000)
            d["recon_x"], d["recon_y"] = x, y
            d["qparam_index"] = 3 * (g % len(fu.QINDICES)) + np.arange(3)
            d["tx_type_y"], d["tx_type_uv"] = types_y[int(rng.integers(0, len(types_y)))], types_uv[int(rng.integers(0, len(types_uv)))]
            d["txb_skip_ctx"], d["dc_sign_ctx"] = rng.integers(0, 13, 3), rng.integers(0, 3, 3)
            if inter:
                d["intra_mode"] = 0
                if kind == "MERGE":
                    f["merge_rate"], d["skip_mode_rate"] = rng.integers(100, 6000), rng.integers(20, 3000)
                    if n_groups < 3:            # reaches the full loop (eob 0) and loses there: an intra candidate wins the block
                        d["luma_rate"] = d["skip_mode_rate"] = 40000000
                pus.append((row, _inter_pu(rng, s, kind, x, y, px, py, has_uv, far=kind != "MERGE" and len(pus) % 5 == 2)))
            else:
                mode = INTRA_MODE[kind] if kind in INTRA_MODE else DIRECTIONAL[(g + j) % len(DIRECTIONAL)]
                s.luma_mode[row] = mode
                s.uv_mode[row] = (iu.DC, 0) if kind == "DC" or (g + j) % 2 else mode
                d["intra_mode"] = mode[0]
            s.kind.append(kind)
            row += 1
    if refusals:
        groups[n_groups // 2]["buffer_total_count"] = 0           # the pick refuses it, and the full loop again
        k = next(i for i, (r, p) in enumerate(pus) if fast[r]["has_uv"] and s.kind[r] in ("BI", "BIw"))
        pus[k][1]["nb_is_inter"][2] = 1                           # BI_PRED whose chroma goes sub-8x8: the prediction refuses it
        s.refused_pu_row = pus[k][0]
    # the candidates the reference would search first: both sides above 4, av1_is_interp_needed (no merge candidate)
    searched = [(r, p) for r, p in pus if ifs and s.kind[r] != "MERGE"]
    rest = [(r, p) for r, p in pus if not (ifs and s.kind[r] != "MERGE")]
    s.n_search = len(searched)
    s.pu_row = np.array([r for r, _ in searched + rest], np.int64)
    s.pu = np.array([p for _, p in searched + rest], svtav1_hip.INTER_PU_DESC_DTYPE).reshape(-1)
    s.ifs_desc = np.zeros(s.n_search, su.IFS_DESC_DTYPE)
    for i in range(s.n_search):
        f = s.ifs_desc[i]
        f["src_x"], f["src_y"] = s.pu[i]["pu_origin_x"], s.pu[i]["pu_origin_y"]
        if i % 3 == 0:          # the rates decide: one of the trials both modes reach (0, 3, 6) costs nothing, the others a lot
            t = (3, 6, 0)[i // 3 % 3]
            f["lambda_"] = su.FORCE_LAMBDA
            f["filter_rate"] = [[0 if k == t // 3 else su.FORCE_RATE + 13 * k for k in range(3)], [0 if k == t % 3 else su.FORCE_RATE + 7 * k for k in range(3)]]
        else:                   # the distortion decides
            f["lambda_"] = rng.integers(500, 4000)
            f["filter_rate"] = rng.integers(20, 400, (2, 3))
    s.fast, s.full, s.groups = fast, full, groups
    s.picks = None
    s.n_slots = n_groups * MAX_FULL
    slot_rows = (s.n_slots + fu.SLOT_TILES_PER_ROW - 1) // fu.SLOT_TILES_PER_ROW
    s.slot_shape = [(slot_rows * s.th, fu.SLOT_TILES_PER_ROW * s.tw)] + [(slot_rows * s.th // 2, fu.SLOT_TILES_PER_ROW * s.tw // 2)] * 2
    s.recon_shape = [p.shape for p in s.src]
    s.alpha_bits = cu.random_alpha_bits(rng)
    return s


def _inter_pu(rng, s, kind, x, y, px, py, has_uv, far):
    w, h = s.w, s.h
    d = np.zeros((), svtav1_hip.INTER_PU_DESC_DTYPE)
    d["pu_origin_x"], d["pu_origin_y"], d["dst_origin_x"], d["dst_origin_y"] = x, y, px, py
    d["mb_to_left_edge"], d["mb_to_right_edge"] = -x * 8, (PIC_W - w - x) * 8
    d["mb_to_top_edge"], d["mb_to_bottom_edge"] = -y * 8, (PIC_H - h - y) * 8
    # with a filter search the search writes the filters; without one the descriptors carry them
    d["interp_filters"] = 0 if s.ifs else (int(rng.integers(0, 3)) << 16) | int(rng.integers(0, 3))
    direction = 2 if kind in ("BI", "BIw") else 1 if kind in ("L1f", "L1w") else 0
    d["pred_direction"], d["has_uv"], d["own_list"] = direction, has_uv, int(direction == 1)
    for k in range(2):
        if kind == "MERGE":
            mv = EXACT_MV
        elif far:               # far enough out to be clamped
            mv = (int(rng.choice([-1, 1])) * int(rng.integers(8 * (PIC_H + 40), 8 * (PIC_H + 200))),
                  int(rng.choice([-1, 1])) * int(rng.integers(8 * (PIC_W + 40), 8 * (PIC_W + 200))))
        elif kind.endswith("w"):
            mv = (16 * int(rng.integers(-2, 3)), 16 * int(rng.integers(-2, 3)))
        else:
            mv = (4 + int(rng.integers(-3, 4)) - 14 * k, 4 + int(rng.integers(-3, 4)) + 10 * k)   # list 1 lies (1.75, -1.25) away
        d["mv"][k] = mv
    for k in range(3):
        d["nb_is_inter"][k] = int(rng.random() < 0.7)
        d["nb_list"][k] = int(rng.integers(0, 2))
        d["nb_mv"][k] = (int(rng.integers(-60, 61)), int(rng.integers(-60, 61)))
    if direction == 2 and ipu.sub8x8(d, w, h):
        d["nb_is_inter"][2 if w == 4 else 1] = 0
    return d


def intra_descs(s, plane, edge_stride, edge_base, dst_stride, dst_base):
    """INTRA_DESC_DTYPE of every intra candidate for `plane` (0 Y: the block's TxSize; 1 Cb, 2 Cr: txsize_uv, candidates with has_uv), the
    edges read from the neighbour picture's plane at `edge_base` + row * `edge_stride`, the block written at its pool tile.
    Returns (descriptors, TxSize)"""
    (bw, bh), ts = ((s.w, s.h), s.ts_y) if plane == 0 else ((s.cw, s.ch), s.ts_uv)
    pw, ph = PIC_W >> (plane > 0), PIC_H >> (plane > 0)
    rows = [r for r in range(s.n_cand) if not s.fast[r]["flags"] & mu.TYPE_INTER and (plane == 0 or s.fast[r]["has_uv"])]
    d = np.zeros(len(rows), iu.DESC)
    for i, r in enumerate(rows):
        f = s.fast[r]
        x, y, px, py = (int(f[k]) for k in ("src_x", "src_y", "pred_x", "pred_y"))
        if plane:
            x, y, px, py = (mu.round_uv(v) for v in (x, y, px, py))
        nt, nl = (bw if y > 0 else 0), (bh if x > 0 else 0)
        d[i]["above_offset"], d[i]["left_offset"], d[i]["left_stride"] = edge_base + (y - 1) * edge_stride + x, edge_base + y * edge_stride + x - 1, edge_stride
        d[i]["dst_offset"], d[i]["dst_stride"] = dst_base + py * dst_stride + px, dst_stride
        d[i]["n_top_px"], d[i]["n_left_px"] = nt, nl
        d[i]["n_topright_px"] = max(0, min(bw, pw - x - bw)) if nt else 0
        d[i]["n_bottomleft_px"] = max(0, min(bh, ph - y - bh)) if nl else 0
        d[i]["mode"], d[i]["angle_delta"] = s.luma_mode[r] if plane == 0 else s.uv_mode[r]
    return d, ts


def slot_rows(s, picks):
    """the host's first look-up: the candidate row each of the n_groups * max_full slots holds, read from the picks (NONE: inactive)"""
    keep, s.picks = s.picks, picks
    out = []
    for k in range(s.n_slots):
        g, i = divmod(k, s.max_full)
        out.append(fu.slot_row(s, g, i) if i < fu.group_slots(s, g) else NONE)
    s.picks = keep
    return out


def cfl_slots(s, rows):
    """the slots the CfL service applies to: active, the candidate intra with a DC chroma prediction, with chroma, not INVALID"""
    if not s.cfl:
        return []
    return [k for k, r in enumerate(rows) if r != NONE and not s.fast[r]["flags"] & (mu.TYPE_INTER | mu.INVALID) and s.fast[r]["has_uv"]
            and s.uv_mode[r][0] == iu.DC]


def cfl_descs(s, slots, rows, luma_stride, luma_base, chroma_stride, chroma_base):
    """CFL_DESC_DTYPE of the slots: luma at the slot's tile of slot_recon.y, the DC tiles in the pool's chroma planes"""
    d = np.zeros(len(slots), cu.DESC)
    for i, k in enumerate(slots):
        tx, ty = fu.tile_xy(s, k)
        qx, qy = (mu.round_uv(int(s.fast[rows[k]][n])) for n in ("pred_x", "pred_y"))
        d[i]["luma_offset"], d[i]["luma_stride"] = luma_base + ty * luma_stride + tx, luma_stride
        d[i]["cb_offset"] = d[i]["cr_offset"] = chroma_base + qy * chroma_stride + qx
        d[i]["chroma_stride"] = chroma_stride
    return d


def cfl_tu_descs(s, slots, rows, src_stride, cb_base, cr_base):
    """(TU_DESC_DTYPE, COEFF_RATE_DESC_DTYPE, CFL_DECISION_JOB_DTYPE) of the 66 candidate tiles a slot: tile t = (slot * 2 + plane) * 33 +
    alpha against the source's Cb (at `cb_base`) or Cr block, DCT_DCT, the candidate's own quantiser rows and contexts"""
    sh = fu.shared()
    npx = s.cw * s.ch
    n_tu = len(slots) * 66
    tu, rd, jobs = np.zeros(n_tu, svtav1_hip.TU_DESC_DTYPE), np.zeros(n_tu, svtav1_hip.COEFF_RATE_DESC_DTYPE), np.zeros(len(slots), cu.JOB)
    so = int(sh["iscan_offsets"][s.ts_uv, 0])
    for i, k in enumerate(slots):
        f, d = s.fast[rows[k]], s.full[rows[k]]
        sx, sy = mu.round_uv(int(f["src_x"])), mu.round_uv(int(f["src_y"]))
        jobs[i] = (int(d["lambda_"]), CFL_MODE_BITS, DC_MODE_BITS)
        for p in range(2):
            t = slice((i * 2 + p) * 33, (i * 2 + p + 1) * 33)
            tu["src_offset"][t] = (cb_base, cr_base)[p] + sy * src_stride + sx
            tu["qparam_index"][t] = d["qparam_index"][1 + p]
            rd["txb_skip_ctx"][t], rd["dc_sign_ctx"][t] = min(int(d["txb_skip_ctx"][1 + p]), 12), min(int(d["dc_sign_ctx"][1 + p]), 2)
    t = np.arange(n_tu)
    tu["pred_offset"] = tu["recon_offset"] = tu["coeff_offset"] = rd["coeff_offset"] = t * npx
    tu["src_stride"], tu["pred_stride"], tu["recon_stride"] = src_stride, s.cw, s.cw
    tu["iscan_offset"] = rd["iscan_offset"] = so
    rd["plane_type"] = 1
    return tu, rd, jobs


def cfl_rate(s, decision):
    """the host's second look-up: what a UV_CFL_PRED decision adds to the candidate's chroma_rate"""
    idx, js = int(decision["cfl_alpha_idx"]), int(decision["cfl_alpha_signs"])
    return CFL_MODE_BITS + int(s.alpha_bits[js][0][idx >> 4]) + int(s.alpha_bits[js][1][idx & 15])


def apply_cfl_decisions(s, slots, rows, decisions, desc):
    """the descriptors of the blocks decided UV_CFL_PRED, their alphas filled in, and their rows; chroma_rate of those rows is changed"""
    sel = [i for i, o in enumerate(decisions) if int(o["intra_chroma_mode"]) == cu.UV_CFL_PRED]
    out = desc[sel].copy()
    out["alpha_idx"], out["alpha_signs"] = decisions["cfl_alpha_idx"][sel], decisions["cfl_alpha_signs"][sel]
    changed = [rows[slots[i]] for i in sel]
    for i, r in zip(sel, changed):
        s.full[r]["chroma_rate"] += cfl_rate(s, decisions[i])
    return out, changed


# ---------------------------------------------------------------- the chain

def _flat_with_row_above(plane):
    """(flat samples, offset of sample (0, 0)): one row in front, so that the row above row 0 has an offset"""
    return np.concatenate([np.full(plane.shape[1], 0x5A, plane.dtype), plane.reshape(-1)]), plane.shape[1]


def run_chain(s, oracle, write_back=True):
    """every array and plane set of the restated chain on scenario s (which it changes): by the names of STAGES, and `refused` by stage"""
    sh = fu.shared()
    w, h = s.w, s.h
    out, refused = {}, {}
    # 1. the filter search, its filters written back
    out["ifs"] = np.zeros(0, su.IFS_RESULT_DTYPE)
    if s.ifs:
        trials = [su.Trials(s.ref0, s.ref1, tuple(s.src), s.pu[i], s.ifs_desc[i], w, h, QUANTIZER) for i in range(s.n_search)]
        out["ifs"], refused["ifs"] = su.search(trials, 1 if s.ifs == "fast" else 2, 1)
        if write_back:
            s.pu["interp_filters"][:s.n_search] = out["ifs"]["interp_filters"]
    out["pu"] = s.pu.copy()
    # 2. inter prediction, 3. intra prediction, into the pool
    pool = ipu.Picture(s.pool[0], s.pool[1], s.pool[2], 0)
    refused["inter"] = ipu.predict(s.ref0, s.ref1, pool, s.pu, w, h, 8)
    for p in range(3):
        edge, base = _flat_with_row_above(s.nb[p])
        d, ts = intra_descs(s, p, s.nb[p].shape[1], base, s.pool[p].shape[1], 0)
        refused["intra", p] = iu.predict(edge, s.pool[p].reshape(-1), d, ts, 8)[0]
    out["pool_luma"], out["pool_chroma_dc"] = [s.pool[0].copy()], [s.pool[1].copy(), s.pool[2].copy()]
    # 4. fast cost, 5. pick
    out["fast"] = mu.fast_cost(s.src, s.pool, s.fast, w, h)
    out["picks"], refused["pick"] = mu.pick(out["fast"], s.fast, s.groups)
    s.picks = out["picks"]
    # 6. full loop, LUMA
    st = fu.full_loop(oracle, s, fu.LUMA)
    out["slot_luma"] = [st["slot"][0].copy()]
    # 7. the CfL service
    rows = slot_rows(s, s.picks)
    assert rows == [sl["row"] for sl in st["slots"]]
    slots = cfl_slots(s, rows)
    out["cfl"], out["cfl_slots"], out["cfl_rows"] = np.zeros(0, cu.DECISION), slots, []
    if slots:
        npx = s.cw * s.ch
        desc = cfl_descs(s, slots, rows, st["slot"][0].shape[1], 0, s.pool[1].shape[1], 0)
        cand = cu.candidates(st["slot"][0].reshape(-1), s.pool[1].reshape(-1), s.pool[2].reshape(-1), desc, w, h)
        tu, rd, jobs = cfl_tu_descs(s, slots, rows, s.src[1].shape[1], 0, s.src[1].size)
        chain = tq_util.oracle_encode_batch(oracle, {"src": np.concatenate([s.src[1].reshape(-1), s.src[2].reshape(-1)]), "pred": cand.reshape(-1), "desc": tu,
                                                     "qparams": sh["qparams"], "scan": sh["tabs"].scan_pool, "w": s.cw, "h": s.ch, "n": npx, "bit_depth": 8})
        so = int(tu[0]["iscan_offset"])
        bits = np.array([rate_util.coeff_bits(sh["tables"][0], chain["qcoeff"][i * npx:(i + 1) * npx], sh["tabs"].iscan_pool[so:so + npx], int(chain["eob"][i]),
                                              s.ts_uv, 0, 1, int(rd[i]["txb_skip_ctx"]), int(rd[i]["dc_sign_ctx"]), 0, 0, 0) for i in range(len(tu))], np.uint32)
        out.update({"cfl_desc": desc, "cfl_cand": cand, "cfl_tu": tu, "cfl_rd": rd, "cfl_jobs": jobs, "cfl_recon": chain["recon"], "cfl_q": chain["qcoeff"], "cfl_eob": chain["eob"],
                    "cfl_dist": chain["dist"], "cfl_bits": bits})
        out["cfl"] = cu.decide_batch(chain["dist"], bits, rate_util.tx_scale_shift(s.ts_uv), s.alpha_bits, jobs)
        chosen, out["cfl_rows"] = apply_cfl_decisions(s, slots, rows, out["cfl"], desc)
        out["cfl_chosen"] = chosen
        refused["cfl"] = cu.predict(st["slot"][0].reshape(-1), s.pool[1].reshape(-1), s.pool[2].reshape(-1), s.pool[1].reshape(-1), s.pool[2].reshape(-1),
                                    chosen, w, h, 8)
    out["pool_chroma"] = [s.pool[1].copy(), s.pool[2].copy()]
    # 8. full loop, CHROMA | DECIDE
    st = fu.full_loop(oracle, s, fu.CHROMA | fu.DECIDE, st)
    refused["full"] = st["refused"]
    out["result"], out["decision"], out["slot"], out["recon"] = st["result"], st["decision"], st["slot"], st["recon"]
    out["full"], out["state"], out["refused"] = s.full.copy(), st, refused
    return out


@contextlib.contextmanager
def chroma_read_at_half_position():
    """the restatements of the fast cost and the full loop, and intra_descs, taking chroma positions as p / 2 instead of ((p >> 3) << 3) / 2
    (kept inside the picture).  Pool positions are multiples of 8, where the two agree: only source, recon and intra-edge positions move"""
    keep = mu.round_uv, fu.round_uv
    mu.round_uv = fu.round_uv = lambda v: min(int(v) // 2, PIC_W // 2 - 4)
    try:
        yield
    finally:
        mu.round_uv, fu.round_uv = keep


_CHAINS = {}


def chain_of(name, oracle, write_back=True, half_chroma=False):
    """(scenario as the chain left it, the restated chain) of size `name`, computed once with `oracle` (the tests' `oracle` fixture; the
    fixture generator, which runs outside pytest, builds its own) and shared by every caller after that"""
    key = (name, write_back, half_chroma)
    if key not in _CHAINS:
        s = make_scenario(name)
        with (chroma_read_at_half_position() if half_chroma else contextlib.nullcontext()):
            _CHAINS[key] = s, run_chain(s, oracle, write_back)
    return _CHAINS[key]


def total_refused(chain):
    return int(sum(chain["refused"].values()))


# ---------------------------------------------------------------- the conditions on the inputs

def measures(s, chain):
    """the figures behind the conditions, from the restated chain"""
    st = chain["state"]
    active = [k for k, sl in enumerate(st["slots"]) if sl["row"] != NONE]
    clamped = 0
    for d in s.pu:
        for l in ((0, 1) if d["pred_direction"] == 2 else (int(d["pred_direction"]),)):
            clamped += ipu.clamp_mv(d, d["mv"][l][0], d["mv"][l][1], s.w, s.h, 0) != (ipu._i16(int(d["mv"][l][0]) * 2), ipu._i16(int(d["mv"][l][1]) * 2))
    win = [int(r) for r in chain["decision"]["winner_row"] if int(r) != NONE]
    cfl = chain["cfl"]
    both = [o for o in cfl if int(o["intra_chroma_mode"]) == cu.UV_CFL_PRED
            and all(cu.idx_to_alpha(int(o["cfl_alpha_idx"]), int(o["cfl_alpha_signs"]), p) for p in range(2))]
    return {"searched": int(s.n_search), "best_trial_not_0": int((chain["ifs"]["best_trial"] != 0).sum()), "clamped_mvs": int(clamped),
            "groups_full_count_below_count": int(sum(int(p["full_count"]) < int(g["count"]) for p, g in zip(chain["picks"], s.groups))),
            "invalid_among_picks": int(sum(bool(s.fast[st["slots"][k]["row"]]["flags"] & mu.INVALID) for k in active)),
            "inter_winners": int(sum(bool(s.fast[r]["flags"] & mu.TYPE_INTER) for r in win)), "intra_winners": int(sum(not s.fast[r]["flags"] & mu.TYPE_INTER for r in win)),
            "luma_eob_0": int(sum(st["luma"][k]["eob"] == 0 for k in active)), "luma_eob_not_0": int(sum(st["luma"][k]["eob"] != 0 for k in active)),
            "cfl_blocks": len(cfl), "cfl_decisions": int((cfl["intra_chroma_mode"] == cu.UV_CFL_PRED).sum()), "cfl_both_alphas": len(both),
            "dc_decisions": int((cfl["intra_chroma_mode"] == cu.UV_DC_PRED).sum()), "winners_cfl_rewrote": int(sum(r in chain["cfl_rows"] for r in win))}


MEASURES = ("searched", "best_trial_not_0", "clamped_mvs", "groups_full_count_below_count", "invalid_among_picks", "inter_winners", "intra_winners",
            "luma_eob_0", "luma_eob_not_0", "cfl_blocks", "cfl_decisions", "cfl_both_alphas", "dc_decisions", "winners_cfl_rewrote")


def conditions(name, m):
    """what the chain's inputs must satisfy, as {condition: holds}, from measures() (or the fixture's copy of them)"""
    ok = {"an MV is clamped": m["clamped_mvs"] >= 1, "a group has full_count < count": m["groups_full_count_below_count"] >= 1,
          "an INVALID candidate is among the picks": m["invalid_among_picks"] >= 1, "an INTER winner": m["inter_winners"] >= 1,
          "an INTRA winner": m["intra_winners"] >= 1, "a luma eob of 0": m["luma_eob_0"] >= 1, "a luma eob other than 0": m["luma_eob_not_0"] >= 1}
    if SIZES[name][2]:
        ok["a third of the searched candidates leave trial 0"] = m["searched"] > 0 and 3 * m["best_trial_not_0"] >= m["searched"]
    if SIZES[name][3]:
        ok.update({"a UV_CFL_PRED decision with both alphas not 0": m["cfl_both_alphas"] >= 1, "a UV_DC_PRED decision": m["dc_decisions"] >= 1,
                   "a winner whose chroma CfL rewrote": m["winners_cfl_rewrote"] >= 1})
    return ok


# ---------------------------------------------------------------- the fixture

def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def input_digests(s):
    """sha256 of the pictures and of every descriptor array as make_scenario leaves them: the proof that a box regenerated the fixture's input"""
    return {"src": sha256(*s.src), "refs": sha256(s.ref0.y, s.ref0.cb, s.ref0.cr, s.ref1.y, s.ref1.cb, s.ref1.cr), "nb": sha256(*s.nb),
            "desc": sha256(s.pu, s.ifs_desc, s.fast, s.full, s.groups, s.luma_mode, s.uv_mode, s.alpha_bits)}


def small(chain, k):
    """stage k of the chain as bytes rows, for the fixture and the comparison"""
    a = np.ascontiguousarray(chain[k])
    return a.view(np.uint8).reshape(len(a), -1) if len(a) else np.zeros((0, a.dtype.itemsize), np.uint8)


_FIXTURE = {}


def fixture():
    if not _FIXTURE:
        _FIXTURE.update(np.load(FIXTURE))
    return _FIXTURE


def expected(name):
    """what the fixture holds of size `name`: the small arrays whole (as rows of bytes), `digest_<stage>` of every plane set, `sha256_<input>`,
    `refused` and the measures"""
    z = fixture()
    out = {k: z[f"{name}_{k}"] for k in STAGES if k not in PLANE_STAGES}
    for k in PLANE_STAGES:
        out["digest_" + k] = z[f"{name}_digest_{k}"]
    for k in ("src", "refs", "nb", "desc"):
        out["sha256_" + k] = z[f"{name}_sha256_{k}"]
    out["refused"] = int(z[f"{name}_refused"])
    out["measures"] = dict(zip(MEASURES, (int(v) for v in z[f"{name}_measures"])))
    return out


def first_difference(got, want, only=None):
    """the first stage, in chain order, at which `got` (arrays and plane lists by the names of STAGES) is not `want` (expected(), or
    another chain), or among the names `only`: a string naming the stage and where, or None"""
    for k in STAGES:
        if only is not None and k not in only:
            continue
        if k in PLANE_STAGES:
            if k in want:
                for p, (a, b) in enumerate(zip(got[k], want[k])):
                    if not np.array_equal(a, b):
                        at = np.argwhere(a != b)
                        return f"{k}, plane {p}: {len(at)} samples differ, the first at (row, column) {at[0].tolist()}"
            elif not np.array_equal(sha256(*got[k]), want["digest_" + k]):
                return f"{k}: the digest of the planes differs"
        else:
            g, w_ = small(got, k), (want[k] if want[k].dtype == np.uint8 and want[k].ndim == 2 else small(want, k))
            if g.shape != w_.shape:
                return f"{k}: {g.shape[0]} rows of {g.shape[1]} bytes, not {w_.shape[0]} of {w_.shape[1]}"
            if not np.array_equal(g, w_):
                rows = np.flatnonzero((g != w_).any(axis=1))
                return f"{k}: rows {rows[:6].tolist()} differ ({len(rows)} in all)"
    return None
