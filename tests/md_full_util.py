"""Restatement of mode decision's full loop (svthip_md_full_loop_batch_dev) for its tests, the fixture generator and the probe.
AV1PerformFullLoop (Codec/EbProductCodingLoop.c:2004-2307) is composed here from parts the other tests already pin -- the oracle's fused chain
(oracle/binding.py: orc_encode_tu), the coefficient rate and the tx-type decision (tests/rate_util.py) -- with the arithmetic that is new:
Av1TuCalcCostLuma as built with CBF_ZERO_OFF, Av1FullCost, Av1MergeSkipFullCost (Codec/EbRateDistortionCost.c:2152-2230, :1485-1721), the
loop of product_full_mode_decision (Codec/EbModeDecision.c:1989-2012) and the copy of the winner's reconstruction.  tests/golden/md_full.npz
holds what the reference's own leaves return (tests/golden/ref_md_full_driver.c) and this restatement's results for the constructed cases."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np

import md_fast_util as mu
import rate_util
import svtav1_hip
from tq_util import RealTables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "md_full.npz")
U64 = (1 << 64) - 1
NONE = 0xFFFFFFFF
FAST_DTYPE, GROUP_DTYPE, PICK_DTYPE = mu.DESC_DTYPE, mu.GROUP_DTYPE, mu.PICK_DTYPE
FULL_DTYPE, RESULT_DTYPE, DECISION_DTYPE = svtav1_hip.md_full_desc_dtype(), svtav1_hip.md_full_result_dtype(), svtav1_hip.md_full_decision_dtype()
LUMA, CHROMA, DECIDE = svtav1_hip.MD_FULL_LUMA, svtav1_hip.MD_FULL_CHROMA, svtav1_hip.MD_FULL_DECIDE
SLOT_FILL, RECON_FILL = 0x55, 0xAA   # what the slot pool and the reconstructed picture hold before a call
SLOT_TILES_PER_ROW, POOL_TILES_PER_ROW = 5, 8
QINDICES = (60, 140)                  # qparams rows 3 * i + plane


# ------------------------------------------------------------------------------------------------ the new arithmetic

def rdcost(lam, rate, dist):
    """RDCOST (EbRateDistortionCost.h:215-217) in unsigned 64-bit arithmetic"""
    return ((((rate * lam) & U64) + 256 & U64) >> 9) + ((dist << 7) & U64) & U64


def tu_cost_luma(lam, bits, dist):
    """Av1TuCalcCostLuma with CBF_ZERO_OFF (:2152-2230): yZeroCbfCost is ~0 -> (bits, dist[0], yFullCost)"""
    nz_cost = rdcost(lam, bits, dist[0])
    nz = nz_cost < U64
    return (bits if nz else 0), (dist[0] if nz else dist[1]), min(nz_cost, U64)


def full_cost(lam, luma_rate, chroma_rate, y, cb, cr, bits):
    """Av1FullCost (:1485-1563) without its CfL terms (they are in chroma_rate) -> (full_cost, full_lambda_rate, full_cost_luma)"""
    total = (y[0] + cb[0] + cr[0]) & U64
    cost = rdcost(lam, (luma_rate + chroma_rate + sum(bits)) & U64, total)
    return cost, (cost - total) & U64, rdcost(lam, (luma_rate + bits[0]) & U64, y[0])


def merge_skip_cost(lam, luma_rate, chroma_rate, skip_mode_rate, y, cb, cr, bits):
    """Av1MergeSkipFullCost (:1580-1721) -> (full_cost, merge_cost, skip_cost, full_lambda_rate, skip_flag)"""
    merge_dist, skip_dist = (y[0] + cb[0] + cr[0]) & U64, (y[1] + cb[1] + cr[1]) & U64
    merge = rdcost(lam, (luma_rate + chroma_rate + sum(bits)) & U64, merge_dist)
    skip = rdcost(lam, skip_mode_rate, skip_dist)
    flag = skip <= merge
    cost = skip if flag else merge
    return cost, merge, skip, (cost - (skip_dist if flag else merge_dist)) & U64, int(flag)


def mode_decision(costs, is_intra, modes):
    """the loop of product_full_mode_decision over the slots in order -> (winner slot, best_intra_mode or 0xff)"""
    lowest = lowest_intra = U64
    win, best_intra = 0, 0xFF
    for i, c in enumerate(costs):
        if c < lowest_intra and is_intra[i]:
            best_intra, lowest_intra = modes[i], c
        if c < lowest:
            win, lowest = i, c
    return win, best_intra


# ------------------------------------------------------------------------------------------------ geometry and tables

def chroma_size(w, h):
    return max(4, w // 2), max(4, h // 2)


def tx_size_of(w, h):
    return svtav1_hip.TX_SIZES_WH.index((w, h))


def round_uv(v):
    return ((v >> 3) << 3) // 2


def masks_of(w, h, search, reduced=0):
    """(type_mask_inter, type_mask_intra) of the luma TxSize: search 'none' (above ENC_M1), 'm0' or 'm1' (allowed_tx_set_a)"""
    if search == "none":
        return 1, 1
    ts = tx_size_of(w, h)
    return tuple(rate_util.tx_search_type_mask(ts, inter, reduced, int(search == "m1")) for inter in (1, 0))


@functools.lru_cache(maxsize=None)
def shared():
    """the real quantiser rows, scans and rate tables every case uses"""
    tabs = RealTables()
    rows = tabs.rows(8, "inter")
    qparams = np.ascontiguousarray(np.concatenate([rows[q] for q in QINDICES]))          # [2 * 3][10]
    offsets = np.zeros((19, 16), np.uint32)
    for ts in range(19):
        for tt in range(16):
            if int(tabs.scan_index[ts, tt]) >= 0:
                offsets[ts, tt] = tabs.scan_offset(ts, tt)
    z = np.load(os.path.join(ROOT, "tests", "golden", "coeff_rate.npz"))
    tables = z["tables"].view(svtav1_hip.COEFF_RATE_TABLES_DTYPE).reshape(-1)[1:2].copy()
    return {"tabs": tabs, "qparams": qparams, "iscan_offsets": offsets, "tables": tables}


# ------------------------------------------------------------------------------------------------ constructed cases

SIZES = ((4, 4), (4, 16), (8, 8), (16, 8), (32, 32), (64, 16), (64, 64))
# name -> (size, n_groups, max_full, search, a group the pick refuses)
CASES = {f"{w}x{h}": ((w, h), 5, 4, s, r) for (w, h), s, r in zip(SIZES, ("m0", "m1", "m0", "none", "m0", "none", "m0"), (0, 0, 1, 0, 0, 1, 0))}
CASES.update({"8x8_g1_m12": ((8, 8), 1, 12, "m1", 0), "8x8_g23_m12": ((8, 8), 23, 12, "m1", 1), "16x8_g5_m1": ((16, 8), 5, 1, "m0", 0),
              "16x8_g5_m12_none": ((16, 8), 5, 12, "none", 0)})


class Scenario:
    """one call's inputs: planes, candidates, picks, descriptors"""


def _texture(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(128 + 70 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.normal(0, 6, (h, w)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scenario(name):
    (w, h), n_groups, max_full, search, refuse = CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 7 + 1)
    s = Scenario()
    s.name, s.w, s.h, s.n_groups, s.max_full = name, w, h, n_groups, max_full
    s.cw, s.ch = chroma_size(w, h)
    s.reduced = int(n_groups == 1)
    s.mask_inter, s.mask_intra = masks_of(w, h, search, s.reduced)
    s.tw, s.th = max(8, w), max(8, h)
    cols = 2 if w == 4 else 4
    s.block_xy = [((g % cols) * w, (g // cols) * h) for g in range(n_groups)]
    pic_w = -(-cols * w // 8) * 8
    pic_h = -(-((n_groups + cols - 1) // cols) * h // 8) * 8
    s.src = [_texture(rng, pic_h, pic_w), _texture(rng, pic_h // 2, pic_w // 2), _texture(rng, pic_h // 2, pic_w // 2)]

    counts = rng.integers(1, 8, n_groups)
    n_cand = int(counts.sum())
    s.n_cand = n_cand
    fast, full = np.zeros(n_cand, FAST_DTYPE), np.zeros(n_cand, FULL_DTYPE)
    pool_rows = (n_cand + POOL_TILES_PER_ROW - 1) // POOL_TILES_PER_ROW
    s.pool = [np.full((pool_rows * s.th, POOL_TILES_PER_ROW * s.tw), 0x11, np.uint8)] + \
             [np.full((pool_rows * s.th // 2, POOL_TILES_PER_ROW * s.tw // 2), 0x11, np.uint8) for _ in range(2)]
    types_y = svtav1_hip.valid_tx_types(w, h)
    types_uv = svtav1_hip.valid_tx_types(s.cw, s.ch)
    groups = np.zeros(n_groups, GROUP_DTYPE)
    row = 0
    for g in range(n_groups):
        x, y = s.block_xy[g]
        has_uv = 1
        if (w, h) == (4, 4):
            has_uv = int(bool(x & 4) and bool(y & 4))
        elif w == 4:
            has_uv = int(bool(x & 4))
        elif h == 4:
            has_uv = int(bool(y & 4))
        groups[g] = (row, counts[g], rng.integers(1, 13), 13)
        for _ in range(int(counts[g])):
            px, py = (row % POOL_TILES_PER_ROW) * s.tw, (row // POOL_TILES_PER_ROW) * s.th
            kind = int(rng.integers(0, 6))   # 0: the source itself (eob 0 everywhere); else noise of growing strength
            for p, (bw_, bh_) in enumerate(((w, h), (s.cw, s.ch), (s.cw, s.ch))):
                sx, sy, qx, qy = (x, y, px, py) if p == 0 else (round_uv(x), round_uv(y), round_uv(px), round_uv(py))
                blk = s.src[p][sy:sy + bh_, sx:sx + bw_].astype(np.int32)
                if kind:
                    blk = blk + rng.normal(0, 3 * kind, blk.shape) + kind * np.sin(np.arange(bw_) / 2.0)[None, :]
                s.pool[p][qy:qy + bh_, qx:qx + bw_] = np.clip(blk, 0, 255)
            inter = int(rng.random() < 0.6)
            f, d = fast[row], full[row]
            f["src_x"], f["src_y"], f["pred_x"], f["pred_y"], f["has_uv"] = x, y, px, py, has_uv
            f["flags"] = (mu.TYPE_INTER if inter else 0) | (mu.INVALID if rng.random() < 0.12 else 0)
            f["rate"], f["merge_rate"], f["lambda_"] = rng.integers(100, 9000), mu.NO_MERGE, rng.integers(500, 4000)
            d["luma_rate"], d["chroma_rate"] = rng.integers(50, 30000), rng.integers(10, 9000)
            d["skip_mode_rate"] = rng.integers(20, 3000) if inter and rng.random() < 0.5 else NONE
            d["lambda_"] = rng.integers(1000, 400000)
            d["recon_x"], d["recon_y"] = x, y
            d["qparam_index"] = 3 * int(rng.integers(0, len(QINDICES))) + np.arange(3)
            d["tx_type_y"], d["tx_type_uv"] = types_y[int(rng.integers(0, len(types_y)))], types_uv[int(rng.integers(0, len(types_uv)))]
            d["txb_skip_ctx"], d["dc_sign_ctx"] = rng.integers(0, 13, 3), rng.integers(0, 3, 3)
            d["intra_mode"] = rng.integers(0, 13)
            row += 1
    if refuse:
        groups[n_groups // 2]["buffer_total_count"] = 0      # a group the pick refuses
    result = np.zeros(n_cand, mu.RESULT_DTYPE)
    result["cost"] = rng.integers(1000, 1 << 40, n_cand)
    result["cost"][(fast["flags"] & mu.INVALID) != 0] = mu.MAX_COST
    s.fast, s.full, s.groups = fast, full, groups
    s.picks, s.pick_refused = mu.pick(result, fast, groups)
    assert s.pick_refused == refuse
    s.n_slots = n_groups * max_full
    slot_rows = (s.n_slots + SLOT_TILES_PER_ROW - 1) // SLOT_TILES_PER_ROW
    s.slot_shape = [(slot_rows * s.th, SLOT_TILES_PER_ROW * s.tw)] + [(slot_rows * s.th // 2, SLOT_TILES_PER_ROW * s.tw // 2)] * 2
    s.recon_shape = [p.shape for p in s.src]
    return s


def fresh_planes(s):
    """(slot planes, reconstructed picture) as they are before a call"""
    return [np.full(sh, SLOT_FILL, np.uint8) for sh in s.slot_shape], [np.full(sh, RECON_FILL, np.uint8) for sh in s.recon_shape]


# ------------------------------------------------------------------------------------------------ the full loop

def group_slots(s, g):
    """the active slot count of group g (:2573), 0 for a group the pick refused"""
    grp, p = s.groups[g], s.picks[g]
    if not mu.group_valid(grp, s.n_cand) or int(p["full_count"]) == 0:
        return 0
    return min(int(p["full_count"]), int(grp["count"]), int(grp["buffer_total_count"]), s.max_full)


def slot_row(s, g, i):
    b = int(s.picks[g]["best"][i])
    if b >= 13:
        return NONE
    c = int(s.picks[g]["buffer_cand"][b])
    return int(s.groups[g]["first"]) + c if c < int(s.groups[g]["count"]) else NONE


def _type_valid(w, h, t):
    return t < 16 and t in svtav1_hip.valid_tx_types(w, h)


def _orc(oracle):
    f = oracle.lib.orc_encode_tu
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8
    return f


def _chain(orc, sh, src, sx, sy, pred, px, py, w, h, tx_type, qrow, ts):
    """the fused chain on one TU -> (recon [h][w], levels, eob, energy, dist0, dist1)"""
    n = min(w, 32) * min(h, 32)
    so = int(sh["iscan_offsets"][ts, tx_type])
    scan = np.ascontiguousarray(sh["tabs"].scan_pool[so:so + n])
    qp = np.ascontiguousarray(sh["qparams"][qrow])
    recon = np.zeros((h, w), np.uint8)
    coeff, q, dq = (np.zeros(n, np.int32) for _ in range(3))
    eob, energy, dist = np.zeros(1, np.uint16), np.zeros(1, np.uint64), np.zeros(2, np.uint64)
    orc(src.ctypes.data + sy * src.strides[0] + sx, src.strides[0], pred.ctypes.data + py * pred.strides[0] + px, pred.strides[0], recon.ctypes.data, w, w, h,
        tx_type, qp.ctypes.data, scan.ctypes.data, coeff.ctypes.data, q.ctypes.data, dq.ctypes.data, eob.ctypes.data, energy.ctypes.data, dist.ctypes.data)
    return recon, q, int(eob[0]), int(energy[0]), int(dist[0]), int(dist[1])


def _bits(sh, q, eob, ts, tx_type, plane, d, inter, reduced):
    n = q.size
    so = int(sh["iscan_offsets"][ts, tx_type])
    return rate_util.coeff_bits(sh["tables"][0], q, sh["tabs"].iscan_pool[so:so + n], eob, ts, tx_type, 1 if plane else 0, min(int(d["txb_skip_ctx"][plane]), 12),
                                min(int(d["dc_sign_ctx"][plane]), 2), inter, min(int(d["intra_mode"]), 12), reduced)


def new_state(s):
    slot, recon = fresh_planes(s)
    return {"slot": slot, "recon": recon, "refused": 0, "slots": [None] * s.n_slots, "luma": [None] * s.n_slots, "chroma": [None] * s.n_slots,
            "result": np.zeros(s.n_slots, RESULT_DTYPE), "decision": np.zeros(s.n_groups, DECISION_DTYPE)}


def tile_xy(s, k):
    return (k % SLOT_TILES_PER_ROW) * s.tw, (k // SLOT_TILES_PER_ROW) * s.th


def full_loop(oracle, s, stages=LUMA | CHROMA | DECIDE, state=None):
    """svthip_md_full_loop_batch_dev on scenario s; `state` carries what the device keeps in d_work, slot_recon and recon between calls.
    s.fast, s.full and s.pool are read when a stage needs them, so a caller may change them between two calls as a host would."""
    sh = shared()
    orc = _orc(oracle)
    st = state if state is not None else new_state(s)
    w, h, cw, ch = s.w, s.h, s.cw, s.ch
    ts_y, ts_uv = tx_size_of(w, h), tx_size_of(cw, ch)
    search = (s.mask_inter | s.mask_intra) != 1
    if stages & LUMA:
        for k in range(s.n_slots):
            g, i = divmod(k, s.max_full)
            n_full = group_slots(s, g)
            row = slot_row(s, g, i) if i < n_full else NONE
            use = row
            if use == NONE and n_full:
                use = slot_row(s, g, 0)
            if use == NONE:
                use = 0
            if n_full == 0 and i == 0:
                st["refused"] += 1
            f, d = s.fast[use], s.full[use]
            inter = int(bool(f["flags"] & mu.TYPE_INTER))
            ty, tuv = int(d["tx_type_y"]), int(d["tx_type_uv"])
            if search:
                ty = 0
                if inter:
                    tuv = 0
            bad = not _type_valid(cw, ch, tuv) or not _type_valid(w, h, ty)
            if bad:
                ty = tuv = 0
                st["refused"] += row != NONE
            sx, sy, px, py = int(f["src_x"]), int(f["src_y"]), int(f["pred_x"]), int(f["pred_y"])
            qrow = int(d["qparam_index"][0])
            if search:
                mask = s.mask_inter if inter else s.mask_intra
                outs, cands = {}, {}
                for t in range(16):
                    if mask >> t & 1:
                        outs[t] = _chain(orc, sh, s.src[0], sx, sy, s.pool[0], px, py, w, h, t, qrow, ts_y)
                        rec, q, eob, energy, d0, d1 = outs[t]
                        cands[t] = (eob, energy, d0, d1, _bits(sh, q, eob, ts_y, t, 0, d, inter, s.reduced))
                ty = rate_util.decide(ts_y, int(d["lambda_"]), cands)["tx_type"]
                if inter:
                    tuv = ty
                rec, q, eob, energy, d0, d1 = outs[ty]
                bits = cands[ty][4]
            else:
                rec, q, eob, energy, d0, d1 = _chain(orc, sh, s.src[0], sx, sy, s.pool[0], px, py, w, h, ty, qrow, ts_y)
                bits = _bits(sh, q, eob, ts_y, ty, 0, d, inter, s.reduced)
            tx, ty_ = tile_xy(s, k)
            st["slot"][0][ty_:ty_ + h, tx:tx + w] = rec
            st["slots"][k] = {"row": row, "use": use, "tx_y": ty, "tx_uv": tuv, "bad": bad}
            st["luma"][k] = {"eob": eob, "energy": energy, "dist": (d0, d1), "bits": bits, "dc": int(q[0])}
    if stages & CHROMA:
        for k in range(s.n_slots):
            sl = st["slots"][k]
            f, d = s.fast[sl["use"]], s.full[sl["use"]]
            inter = int(bool(f["flags"] & mu.TYPE_INTER))
            sx, sy, px, py = (round_uv(int(f[n])) for n in ("src_x", "src_y", "pred_x", "pred_y"))
            tx, ty_ = (v // 2 for v in tile_xy(s, k))
            out = []
            for p in (1, 2):
                rec, q, eob, _, d0, d1 = _chain(orc, sh, s.src[p], sx, sy, s.pool[p], px, py, cw, ch, sl["tx_uv"], int(d["qparam_index"][p]), ts_uv)
                st["slot"][p][ty_:ty_ + ch, tx:tx + cw] = rec
                out.append({"eob": eob, "dist": (d0, d1), "bits": _bits(sh, q, eob, ts_uv, sl["tx_uv"], p, d, inter, s.reduced), "dc": int(q[0])})
            st["chroma"][k] = out
    if stages & DECIDE:
        shift_y, shift_uv = rate_util.tx_scale_shift(ts_y), rate_util.tx_scale_shift(ts_uv)
        res = st["result"]
        res[:] = np.zeros(1, RESULT_DTYPE)[0]
        for k in range(s.n_slots):
            sl, r = st["slots"][k], res[k]
            r["row"], r["tx_type_y"], r["tx_type_uv"], r["full_cost"] = sl["row"], sl["tx_y"], sl["tx_uv"], U64
            if sl["row"] == NONE:
                continue
            f, d = s.fast[sl["row"]], s.full[sl["row"]]
            if (f["flags"] & mu.INVALID) or sl["bad"]:
                continue
            lam, lu = int(d["lambda_"]), st["luma"][k]
            y = [(v + lu["energy"] & U64) >> shift_y if shift_y >= 0 else (v + lu["energy"] << -shift_y) & U64 for v in lu["dist"]]
            y_bits, y[0], _ = tu_cost_luma(lam, lu["bits"], y)
            cb, cr, bits, eobs, dcs = [0, 0], [0, 0], [y_bits, 0, 0], [lu["eob"], 0, 0], [lu["dc"], 0, 0]
            if f["has_uv"]:
                for p, dist in ((1, cb), (2, cr)):
                    c = st["chroma"][k][p - 1]
                    dist[:] = [v >> shift_uv if shift_uv >= 0 else (v << -shift_uv) & U64 for v in c["dist"]]
                    bits[p], eobs[p], dcs[p] = c["bits"], c["eob"], c["dc"]
            r["y_distortion"], r["cb_distortion"], r["cr_distortion"], r["coeff_bits"], r["eob"], r["quantized_dc"] = y, cb, cr, bits, eobs, dcs
            r["y_has_coeff"], r["u_has_coeff"], r["v_has_coeff"] = (int(e != 0) for e in eobs)
            r["block_has_coeff"] = int(any(eobs))
            if int(d["skip_mode_rate"]) == NONE:
                r["full_cost"], r["full_lambda_rate"], r["full_cost_luma"] = full_cost(lam, int(d["luma_rate"]), int(d["chroma_rate"]), y, cb, cr, bits)
            else:
                r["full_cost"], r["merge_cost"], r["skip_cost"], r["full_lambda_rate"], r["skip_flag"] = merge_skip_cost(
                    lam, int(d["luma_rate"]), int(d["chroma_rate"]), int(d["skip_mode_rate"]), y, cb, cr, bits)
        dec = st["decision"]
        for g in range(s.n_groups):
            n_full = group_slots(s, g)
            dec[g] = (U64, NONE, 0xFF, 0xFF, 0xFF, n_full)
            if n_full == 0:
                continue
            rows = res[g * s.max_full:g * s.max_full + n_full]
            intra = [int(r["row"]) != NONE and not (s.fast[int(r["row"])]["flags"] & mu.TYPE_INTER) for r in rows]
            modes = [int(s.full[int(r["row"])]["intra_mode"]) if int(r["row"]) != NONE else 0 for r in rows]
            win, best_intra = mode_decision([int(c) for c in rows["full_cost"]], intra, modes)
            dec[g] = (rows[win]["full_cost"], rows[win]["row"], win, s.picks[g]["best"][win], best_intra, n_full)
            wrow = int(rows[win]["row"])
            if wrow == NONE:
                continue
            f, d = s.fast[wrow], s.full[wrow]
            tx, ty_ = tile_xy(s, g * s.max_full + win)
            rx, ry = int(d["recon_x"]), int(d["recon_y"])
            st["recon"][0][ry:ry + h, rx:rx + w] = st["slot"][0][ty_:ty_ + h, tx:tx + w]
            if f["has_uv"]:
                for p in (1, 2):
                    st["recon"][p][round_uv(ry):round_uv(ry) + ch, round_uv(rx):round_uv(rx) + cw] = st["slot"][p][ty_ // 2:ty_ // 2 + ch, tx // 2:tx // 2 + cw]
    return st


def digest(planes):
    return hashlib.sha256(b"".join(np.ascontiguousarray(p).tobytes() for p in planes)).hexdigest()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the one-call result of a case, computed once and asserted equal to the fixture"""
    from oracle.binding import Oracle
    st = full_loop(Oracle(), scenario(name))
    fx = fixture()
    assert st["result"].tobytes() == fx[f"{name}__result"].tobytes() and st["decision"].tobytes() == fx[f"{name}__decision"].tobytes(), f"{name}: the restatement left the fixture"
    assert [digest(st["slot"]), digest(st["recon"])] == [str(v) for v in fx[f"{name}__digests"]] and st["refused"] == int(fx[f"{name}__refused"])
    return st


_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = dict(np.load(FIXTURE))
    return _FIXTURE


# ------------------------------------------------------------------------------------------------ the reference's leaves

def leaf_tuples(n=300, seed=11):
    """random inputs of the leaves: merge candidates on both sides of skip_cost <= merge_cost, equal costs, costs of ~0"""
    rng = np.random.default_rng(seed)
    t = {"lam": rng.integers(1, 1 << 20, n), "bits": rng.integers(0, 1 << 22, (n, 3)), "y": rng.integers(0, 1 << 34, (n, 2)),
         "cb": rng.integers(0, 1 << 30, (n, 2)), "cr": rng.integers(0, 1 << 30, (n, 2)), "luma_rate": rng.integers(0, 1 << 20, n),
         "chroma_rate": rng.integers(0, 1 << 18, n), "skip_rate": rng.integers(0, 1 << 14, n), "inter": rng.integers(0, 2, n),
         "merge": rng.integers(0, 2, n), "has_uv": rng.integers(0, 2, n), "eob": rng.integers(0, 3, (n, 3)), "zero_bits": rng.integers(0, 5000, n),
         "skip_ctx": rng.integers(0, 3, n), "txb_ctx": rng.integers(0, 13, n), "tx_size": rng.integers(0, 19, n)}
    t = {k: v.astype(np.uint64) for k, v in t.items()}
    k = np.arange(n)
    t["y"][k % 4 == 1, 1] = t["y"][k % 4 == 1, 0] >> 3           # a prediction distortion far below the residual's: skip wins
    t["y"][k % 16 == 2] = (1 << 57) - 1                           # costs that wrap
    same = k % 8 == 3                                             # skip_cost == merge_cost exactly
    t["y"][same, 1], t["cb"][same, 1], t["cr"][same, 1] = t["y"][same, 0], t["cb"][same, 0], t["cr"][same, 0]
    t["bits"][same], t["luma_rate"][same], t["chroma_rate"][same] = 0, t["skip_rate"][same], 0
    return t


def decision_lists(n=120, seed=12):
    """(costs [n][12], types [n][12] 1 INTER / 2 INTRA, modes, order [n][12], count [n]) with equal costs and all-~0 lists"""
    rng = np.random.default_rng(seed)
    costs = rng.integers(0, 40, (n, 12)).astype(np.uint64) * 1000
    costs[rng.random((n, 12)) < 0.15] = U64
    costs[::10] = U64
    types = rng.integers(1, 3, (n, 12)).astype(np.uint8)
    types[5::10] = 1
    modes = rng.integers(0, 13, (n, 12)).astype(np.uint8)
    order = np.stack([rng.permutation(12) for _ in range(n)]).astype(np.uint8)
    return costs, types, modes, order, rng.integers(1, 13, n)


def leaves(t):
    """the restatement on leaf_tuples -> {name: array}"""
    n = len(t["lam"])
    out = {"luma": np.zeros((n, 3), np.uint64), "cost": np.zeros((n, 6), np.uint64)}
    for i in range(n):
        lam, bits = int(t["lam"][i]), [int(v) for v in t["bits"][i]]
        y, cb, cr = ([int(v) for v in t[k][i]] for k in ("y", "cb", "cr"))
        out["luma"][i] = tu_cost_luma(lam, bits[0], y)
        lr, crr = int(t["luma_rate"][i]), int(t["chroma_rate"][i])
        if t["inter"][i] and t["merge"][i]:
            c, m, s_, lrate, flag = merge_skip_cost(lam, lr, crr, int(t["skip_rate"][i]), y, cb, cr, bits)
            out["cost"][i] = (c, m, s_, lrate, 0, flag)
        else:
            c, lrate, cl = full_cost(lam, lr, crr, y, cb, cr, bits)
            out["cost"][i] = (c, 0, 0, lrate, cl, 0)
    return out


def decisions(lists):
    costs, types, modes, order, count = lists
    out = np.zeros((len(costs), 3), np.uint64)
    for i in range(len(costs)):
        o = order[i][:count[i]]
        win, best_intra = mode_decision([int(costs[i][b]) for b in o], [types[i][b] == 2 for b in o], [int(modes[i][b]) for b in o])
        out[i] = (o[win], best_intra, costs[i][o[win]])
    return out


def build_reference_driver(out_dir):
    from oracle import ref_driver
    L = ref_driver.build_driver(os.path.join(ROOT, "tests", "golden", "ref_md_full_driver.c"), out_dir)
    V = C.c_void_p
    L.drv_md_full_tu_cost_luma.argtypes = [C.c_int, C.c_int, C.c_uint32, V, V, C.c_uint64, C.c_int32, V, V]
    L.drv_md_full_tu_cost.argtypes = [C.c_int, C.c_int, V, V, V, V, V, C.c_uint64, V]
    L.drv_md_full_cost.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_int32, V, V, V, C.c_uint64, V, V]
    L.drv_md_full_decision.argtypes = [C.c_int, V, V, V, V, C.c_uint32, V, V]
    return L


def reference_leaves(L, t):
    """the reference's own functions on leaf_tuples -> {name: array}, has_coeff [n][3] of Av1TuCalcCostLuma / Av1TuCalcCost included"""
    n = len(t["lam"])
    out = {"luma": np.zeros((n, 3), np.uint64), "cost": np.zeros((n, 6), np.uint64), "has_coeff": np.zeros((n, 3), np.uint32)}
    for i in range(n):
        lam = int(t["lam"][i])
        y, bits = t["y"][i].copy(), t["bits"][i].copy()
        cost, yh = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
        assert L.drv_md_full_tu_cost_luma(int(t["txb_ctx"][i]), int(t["tx_size"][i]), int(t["eob"][i][0]), y.ctypes.data, bits.ctypes.data, lam,
                                          int(t["zero_bits"][i]), cost.ctypes.data, yh.ctypes.data) == 0
        out["luma"][i] = (bits[0], y[0], cost[0])
        y2, cb, cr, b2 = t["y"][i].copy(), t["cb"][i].copy(), t["cr"][i].copy(), t["bits"][i].copy()
        counts, hc = np.ascontiguousarray(t["eob"][i].astype(np.uint32)), np.zeros(3, np.uint32)
        assert L.drv_md_full_tu_cost(int(t["txb_ctx"][i]), int(t["tx_size"][i]), counts.ctypes.data, y2.ctypes.data, cb.ctypes.data, cr.ctypes.data,
                                     b2.ctypes.data, lam, hc.ctypes.data) == 0
        assert np.array_equal(cb, t["cb"][i]) and np.array_equal(cr, t["cr"][i]) and np.array_equal(b2, t["bits"][i])   # chroma numbers stand
        out["has_coeff"][i] = (yh[0], hc[1], hc[2])
        y3, b3, o = t["y"][i].copy(), t["bits"][i].copy(), np.zeros(6, np.uint64)
        assert L.drv_md_full_cost(int(t["inter"][i]), int(t["merge"][i]), int(t["has_uv"][i]), int(t["luma_rate"][i]), int(t["chroma_rate"][i]),
                                  int(t["skip_ctx"][i]), int(t["skip_rate"][i]), y3.ctypes.data, cb.ctypes.data, cr.ctypes.data, lam, b3.ctypes.data,
                                  o.ctypes.data) == 0
        out["cost"][i] = o
    return out


def reference_decisions(L, lists):
    costs, types, modes, order, count = lists
    out = np.zeros((len(costs), 3), np.uint64)
    for i in range(len(costs)):
        bi, oc = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
        c, ty, md, od = (np.ascontiguousarray(a[i]) for a in (costs, types, modes, order))
        win = L.drv_md_full_decision(12, c.ctypes.data, ty.ctypes.data, md.ctypes.data, od.ctypes.data, int(count[i]), bi.ctypes.data, oc.ctypes.data)
        assert win >= 0
        out[i] = (win, bi[0], oc[0])
    return out
