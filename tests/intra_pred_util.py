"""TEST INFRASTRUCTURE: a numpy restatement of the reference's intra prediction of one transform block -- build_intra_predictors /
build_intra_predictors_high (Source/Lib/Codec/EbIntraPrediction.c:8823-9080 / :9082-9317) as configured (no edge filter, no upsampling,
no filter-intra, no palette) -- in the terms of svthip_intra_desc, with the device's refusals.  tests/test_intra_pred_vs_ref.py pins it to
the reference's own outputs (tests/golden/intra_pred.npz, and a live run where the reference exists); the GPU tests hold the device to it.

The edges are always built whole (as generate_intra_reference_samples does for mode decision); the EncDec path's constant fill for a mode
whose only edge is missing gives the same samples: the fixture records both paths' blocks for 608 positions, and they are equal."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "svt-av1-1_amd", "python"), os.path.join(ROOT, "tools")]

import svtav1_hip  # noqa: E402
from gen_intra_tables import derivative_table, weight_table  # noqa: E402

DESC = svtav1_hip.INTRA_DESC_DTYPE
TX_SIZES_WH = svtav1_hip.TX_SIZES_WH
DR = np.array(derivative_table(), np.int64)
SMW = np.array(weight_table(), np.int64)
DC, V, H, D45, D135, D113, D157, D203, D67, SMOOTH, SMOOTH_V, SMOOTH_H, PAETH = range(13)
MODE_ANGLE = [0, 90, 180, 45, 135, 113, 157, 203, 67]
DIRECTIONAL = [(m, d) for m in range(V, D67 + 1) for d in range(-3, 4)]
FILL = {8: 0x55, 10: 0x155}


def new_stats():
    return {"dc_arms": set(), "subst": set(), "z1_tail": 0, "z2_both": 0, "paeth": set(), "zero": 0, "max": 0,
            "partial_top": 0, "partial_left": 0, "topright": set(), "bottomleft": set(), "dir": set(), "modes": set()}


def desc_valid(d, txw, txh):
    nt, ntr, nl, nbl = int(d["n_top_px"]), int(d["n_topright_px"]), int(d["n_left_px"]), int(d["n_bottomleft_px"])
    if int(d["mode"]) > 12 or abs(int(d["angle_delta"])) > 3:
        return False
    if nt > txw or ntr > txw or nl > txh or nbl > txh:
        return False
    return not ((ntr > 0 and nt != txw) or (nbl > 0 and nl != txh))


def build_edges(edge, d, txw, txh, bd, stats=None):
    """above[0 .. N], left[0 .. N] with sample -1 at index 0 (N = txw + txh)"""
    n = txw + txh
    base = 128 << (bd - 8)
    nt, ntr, nl, nbl = int(d["n_top_px"]), int(d["n_topright_px"]), int(d["n_left_px"]), int(d["n_bottomleft_px"])
    ao, lo, ls = int(d["above_offset"]), int(d["left_offset"]), int(d["left_stride"])
    i = np.arange(n)
    if nt > 0:
        above = edge[ao + np.minimum(i, nt + ntr - 1)].astype(np.int64)
    else:
        above = np.full(n, int(edge[lo]) if nl > 0 else base - 1, np.int64)
    if nl > 0:
        left = edge[lo + np.minimum(i, nl + nbl - 1) * ls].astype(np.int64)
    else:
        left = np.full(n, int(edge[ao]) if nt > 0 else base + 1, np.int64)
    if nt > 0 and nl > 0:
        corner = int(edge[ao - 1])
    elif nt > 0:
        corner = int(edge[ao])
    elif nl > 0:
        corner = int(edge[lo])
    else:
        corner = base
    if stats is not None:
        stats["subst"].add(("above", "own" if nt > 0 else "left0" if nl > 0 else "base-1"))
        stats["subst"].add(("left", "own" if nl > 0 else "above0" if nt > 0 else "base+1"))
        stats["subst"].add(("corner", "own" if nt > 0 and nl > 0 else "above0" if nt > 0 else "left0" if nl > 0 else "base"))
        stats["partial_top"] += 0 < nt < txw
        stats["partial_left"] += 0 < nl < txh
        if nt == txw:
            stats["topright"].add("zero" if ntr == 0 else "full" if ntr == txw else "partial")
        if nl == txh:
            stats["bottomleft"].add("zero" if nbl == 0 else "full" if nbl == txh else "partial")
    return np.concatenate([[corner], above]), np.concatenate([[corner], left])


def predict_from_edges(a, lf, mode, delta, txw, txh, have_top, have_left, bd, stats=None):
    """a, lf: edges with sample -1 at index 0.  Returns the txh x txw block (int64)."""
    n = txw + txh
    A, L = a[1:], lf[1:]
    r = np.arange(txh)[:, None]
    c = np.arange(txw)[None, :]
    kind = mode
    p = 0
    if V <= mode <= D67:
        p = MODE_ANGLE[mode] + 3 * delta
        kind = V if p == 90 else H if p == 180 else "z1" if p < 90 else "z2" if p < 180 else "z3"
        if stats is not None:
            stats["dir"].add((mode, delta))
    if stats is not None:
        stats["modes"].add(mode)
    if kind == DC:
        if have_top and have_left:
            v = (A[:txw].sum() + L[:txh].sum() + (n >> 1)) // n
        elif have_top:
            v = (A[:txw].sum() + (txw >> 1)) // txw
        elif have_left:
            v = (L[:txh].sum() + (txh >> 1)) // txh
        else:
            v = 128 << (bd - 8)
        if stats is not None:
            stats["dc_arms"].add((bool(have_left), bool(have_top)))
        out = np.full((txh, txw), v, np.int64)
    elif kind == V:
        out = np.broadcast_to(A[:txw][None, :], (txh, txw)).copy()
    elif kind == H:
        out = np.broadcast_to(L[:txh][:, None], (txh, txw)).copy()
    elif kind == SMOOTH:
        wh, ww = SMW[txh:2 * txh][:, None], SMW[txw:2 * txw][None, :]
        out = (wh * A[:txw][None, :] + (256 - wh) * L[txh - 1] + ww * L[:txh][:, None] + (256 - ww) * A[txw - 1] + 256) >> 9
    elif kind == SMOOTH_V:
        wh = SMW[txh:2 * txh][:, None]
        out = (wh * A[:txw][None, :] + (256 - wh) * L[txh - 1] + 128) >> 8
    elif kind == SMOOTH_H:
        ww = SMW[txw:2 * txw][None, :]
        out = (ww * L[:txh][:, None] + (256 - ww) * A[txw - 1] + 128) >> 8
    elif kind == PAETH:
        top, left, tl = np.broadcast_to(A[:txw][None, :], (txh, txw)), np.broadcast_to(L[:txh][:, None], (txh, txw)), a[0]
        b = top + left - tl
        pl, pt, ptl = np.abs(b - left), np.abs(b - top), np.abs(b - tl)
        take_left = (pl <= pt) & (pl <= ptl)
        take_top = ~take_left & (pt <= ptl)
        out = np.where(take_left, left, np.where(take_top, top, tl))
        if stats is not None:
            tl_b = np.broadcast_to(tl, top.shape)
            # a winner counts where its value differs from both other candidates
            for name, m, mine, o1, o2 in (("left", take_left, left, top, tl_b), ("top", take_top, top, left, tl_b),
                                          ("topleft", ~take_left & ~take_top, tl_b, left, top)):
                if (m & (mine != o1) & (mine != o2)).any():
                    stats["paeth"].add(name)
    elif kind == "z1":
        dx = int(DR[p])
        x = (r + 1) * dx
        b, sh = (x >> 6) + c, (x & 63) >> 1
        mb = n - 1
        val = (A[np.minimum(b, mb)] * (32 - sh) + A[np.minimum(b + 1, mb)] * sh + 16) >> 5
        out = np.where(b < mb, val, A[mb])
        if stats is not None:
            stats["z1_tail"] += bool((b >= mb).any())
    elif kind == "z3":
        # the reference's tail arm (base >= max_base_y) cannot be reached: dy <= 40 for every legal angle, so base < txw * 40 / 64 + txh
        dy = int(DR[270 - p])
        y = (c + 1) * dy
        b, sh = (y >> 6) + r, (y & 63) >> 1
        assert (b < n - 1).all()
        out = (L[b] * (32 - sh) + L[b + 1] * sh + 16) >> 5
    else:
        dx, dy = int(DR[180 - p]), int(DR[p - 90])
        x = -(r + 1) * dx + 0 * c
        b1, sh1 = (x >> 6) + c, (x & 63) >> 1
        y = (r << 6) - (c + 1) * dy
        b2, sh2 = y >> 6, (y & 63) >> 1
        assert (b2[b1 < -1] >= -1).all()
        up = b1 >= -1
        b2 = np.maximum(b2, -1)
        b1c = np.maximum(b1, -1)
        va = (a[b1c + 1] * (32 - sh1) + a[b1c + 2] * sh1 + 16) >> 5
        vl = (lf[b2 + 1] * (32 - sh2) + lf[np.minimum(b2 + 2, n)] * sh2 + 16) >> 5
        out = np.where(up, va, vl)
        if stats is not None:
            stats["z2_both"] += bool((up.any(axis=1) & (~up).any(axis=1)).any())
    if stats is not None:
        stats["zero"] += bool((out == 0).any())
        stats["max"] += bool((out == (1 << bd) - 1).any())
    return out


def predict_block(edge, d, txw, txh, bd, stats=None):
    if not desc_valid(d, txw, txh):
        return None
    a, lf = build_edges(edge, d, txw, txh, bd, stats)
    return predict_from_edges(a, lf, int(d["mode"]), int(d["angle_delta"]), txw, txh, int(d["n_top_px"]) > 0, int(d["n_left_px"]) > 0, bd, stats)


def predict(edge, dst, desc, tx_size, bd, src=None, stats=None):
    """The batch on flat sample arrays (dst may be edge).  Returns (refused, sad): sad[i] against src for valid blocks when src is given."""
    txw, txh = TX_SIZES_WH[tx_size]
    refused = 0
    sad = np.zeros(len(desc), np.uint32)
    rows = np.arange(txh)[:, None]
    cols = np.arange(txw)[None, :]
    for i, d in enumerate(desc):
        blk = predict_block(edge, d, txw, txh, bd, stats)
        if blk is None:
            refused += 1
            continue
        dst[int(d["dst_offset"]) + rows * int(d["dst_stride"]) + cols] = blk.astype(dst.dtype)
        if src is not None:
            s = src[int(d["src_offset"]) + rows * int(d["src_stride"]) + cols].astype(np.int64)
            sad[i] = np.abs(s - blk).sum()
    return refused, sad


def random_case(rng, n, tx_size, bd, n_modes=13, kinds=(0, 1, 2, 3)):
    """n blocks with neighbour-array edges in one flat buffer: per block [pad | -1 | above 0 .. 2 txw) | left 0 .. 2 txh)] and the block's
    destination in a second buffer.  n_modes = 12 leaves PAETH out (the reference has no PAETH predictor).  Counts, modes and deltas are mixed; extremes (0 and the maximum) are frequent."""
    txw, txh = TX_SIZES_WH[tx_size]
    dt = np.uint8 if bd == 8 else np.uint16
    per = 4 + 2 * txw + 2 * txh
    kind = rng.choice(kinds, n)   # 0, 3 noise; 1 noisy ramp; 2 extremes
    edge = rng.integers(0, 1 << bd, n * per).astype(dt)
    e2 = edge.reshape(n, per)
    for i in range(n):
        if kind[i] == 1:      # smooth ramp with noise
            e2[i] = np.clip(rng.integers(0, 1 << bd) + np.cumsum(rng.integers(-3, 4, per)), 0, (1 << bd) - 1)
        elif kind[i] == 2:    # extremes
            e2[i] = rng.choice([0, (1 << bd) - 1], per)
    desc = np.zeros(n, DESC)
    desc["above_offset"] = np.arange(n) * per + 4
    desc["left_offset"] = np.arange(n) * per + 4 + 2 * txw
    desc["left_stride"] = 1
    desc["dst_stride"] = txw
    desc["dst_offset"] = np.arange(n) * txw * txh
    desc["src_stride"] = txw
    desc["src_offset"] = np.arange(n) * txw * txh
    desc["mode"] = rng.integers(0, n_modes, n)
    desc["angle_delta"] = rng.integers(-3, 4, n)
    for i in range(n):
        t = rng.integers(0, 6)
        nt = 0 if t == 0 else txw if t < 4 else rng.integers(1, txw + 1)
        t = rng.integers(0, 6)
        nl = 0 if t == 0 else txh if t < 4 else rng.integers(1, txh + 1)
        ntr = rng.choice([0, txw, rng.integers(1, txw + 1)]) if nt == txw else 0
        nbl = rng.choice([0, txh, rng.integers(1, txh + 1)]) if nl == txh else 0
        desc[i]["n_top_px"], desc[i]["n_topright_px"], desc[i]["n_left_px"], desc[i]["n_bottomleft_px"] = nt, ntr, nl, nbl
    src = rng.integers(0, 1 << bd, n * txw * txh).astype(dt)
    return edge, desc, src


def run_device(ctx, edge, dst, desc, tx_size, bd, src=None, want_sad=False, in_place=False, stream=None):
    """The device entry on flat arrays; returns (dst after the call, sad or None)."""
    import torch
    d_edge = torch.from_numpy(edge.copy()).to("cuda:0") if edge.dtype == np.uint8 else torch.from_numpy(edge.view(np.int16).copy()).to("cuda:0")
    if in_place:
        d_dst = d_edge
    else:
        d_dst = torch.from_numpy(dst.copy()).to("cuda:0") if dst.dtype == np.uint8 else torch.from_numpy(dst.view(np.int16).copy()).to("cuda:0")
    d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_sad = None
    if bd == 8:
        d_src = torch.from_numpy(src.copy()).to("cuda:0") if src is not None else None
        if want_sad:
            d_sad = torch.full((len(desc),), 0xdeadbeef - (1 << 32), dtype=torch.int32, device="cuda:0")
        ctx.av1_intra_pred_batch_dev(d_edge.data_ptr(), d_dst.data_ptr(), d_desc.data_ptr(), len(desc), tx_size,
                                     d_src.data_ptr() if d_src is not None else None, d_sad.data_ptr() if d_sad is not None else None, stream)
    else:
        ctx.av1_highbd_intra_pred_batch_dev(d_edge.data_ptr(), d_dst.data_ptr(), d_desc.data_ptr(), len(desc), tx_size, bd, stream)
    ctx.synchronize()
    out = d_dst.cpu().numpy()
    return (out if bd == 8 else out.view(np.uint16)), (d_sad.cpu().numpy().view(np.uint32) if d_sad is not None else None)
