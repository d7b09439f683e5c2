"""Restatement of mode decision's full loop for the 128-wide blocks (svthip_md_full_loop128_batch_dev) for its tests, the fixture generator
and the probe.  128x128, 128x64 and 64x128 have txb_count = 4, 2, 2 luma TUs of TX_64X64 and per txb_itr one Cb and one Cr TU of TX_32X32
(Codec/EbUtility.c:781-817); ProductFullLoop, FullLoop_R and CuFullDistortionFastTuMode_R loop over txb_itr (Codec/EbFullLoop.c:968-1091,
:1801-1918, :1965-2082) and AV1PerformFullLoop runs no tx-type search (Codec/EbProductCodingLoop.c:2133).  The parts are those of
tests/md_full_util.py -- the oracle's fused chain, the coefficient rate of tests/rate_util.py, Av1TuCalcCostLuma, Av1FullCost,
Av1MergeSkipFullCost, the loop of product_full_mode_decision --; new here is only the walk over the TUs: sums of bits and distortions, the
has_coeff bit masks, the last TU's quantized_dc, eob[plane][tu].  tests/golden/md_full128.npz holds what the reference's own loops return
for these inputs (tests/golden/ref_md_full128_driver.c) and this restatement's results."""
import functools
import os

import numpy as np

import md_fast_util as mu
import md_full_util as fu
import rate_util
import svtav1_hip

ROOT = fu.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "md_full128.npz")
U64, NONE = fu.U64, fu.NONE
LUMA, CHROMA, DECIDE = fu.LUMA, fu.CHROMA, fu.DECIDE
RESULT_DTYPE, DECISION_DTYPE, TU_DTYPE = fu.RESULT_DTYPE, fu.DECISION_DTYPE, svtav1_hip.md_full128_tu_dtype()
SLOT_TILES_PER_ROW, POOL_TILES_PER_ROW = 3, 4
TU, TU_UV = 64, 32                     # every luma TU is TX_64X64, every chroma TU TX_32X32
TS_Y, TS_UV = fu.tx_size_of(TU, TU), fu.tx_size_of(TU_UV, TU_UV)
BAD_UV_TYPE = 1                        # ADST_DCT: 32x32 has no network for it

# name -> (size, n_groups, max_full, a group the pick refuses)
CASES = {"128x128": ((128, 128), 3, 3, 0), "128x64": ((128, 64), 2, 1, 0), "64x128": ((64, 128), 5, 12, 1)}


def tu_origins(w, h):
    """tx_org_x / tx_org_y of the block's luma TUs in the order of txb_itr (EbUtility.c:781-817)"""
    return [(x, y) for y in range(0, h, TU) for x in range(0, w, TU)]


@functools.lru_cache(maxsize=None)
def scenario(name):
    """one call's inputs.  Per TU a candidate's prediction is the source itself (eob 0) or the source plus noise and an offset of its own
    (a DC level of its own), chosen per plane, so that has_coeff masks with some bits set, slots with every eob 0 and TUs whose first levels
    differ all occur; candidate 1 of every group is INVALID or has a tx_type_uv without a network, alternately."""
    (w, h), n_groups, max_full, refuse = CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 11 + 3)
    s = fu.Scenario()
    s.name, s.w, s.h, s.n_groups, s.max_full = name, w, h, n_groups, max_full
    s.cw, s.ch = w // 2, h // 2
    s.reduced = 0
    s.tw, s.th = w, h
    s.origins = tu_origins(w, h)
    cols = 2
    s.block_xy = [((g % cols) * w, (g // cols) * h) for g in range(n_groups)]
    pic_w, pic_h = cols * w, ((n_groups + cols - 1) // cols) * h
    s.src = [fu._texture(rng, pic_h, pic_w), fu._texture(rng, pic_h // 2, pic_w // 2), fu._texture(rng, pic_h // 2, pic_w // 2)]
    counts = rng.integers(3, 7, n_groups)
    n_cand = int(counts.sum())
    s.n_cand = n_cand
    fast, full = np.zeros(n_cand, fu.FAST_DTYPE), np.zeros(n_cand, fu.FULL_DTYPE)
    pool_rows = (n_cand + POOL_TILES_PER_ROW - 1) // POOL_TILES_PER_ROW
    s.pool = [np.full((pool_rows * h, POOL_TILES_PER_ROW * w), 0x11, np.uint8)] + \
             [np.full((pool_rows * h // 2, POOL_TILES_PER_ROW * w // 2), 0x11, np.uint8) for _ in range(2)]
    types_uv = svtav1_hip.valid_tx_types(TU_UV, TU_UV)
    groups = np.zeros(n_groups, fu.GROUP_DTYPE)
    row = 0
    for g in range(n_groups):
        x, y = s.block_xy[g]
        groups[g] = (row, counts[g], rng.integers(2, 13), 13)
        for c in range(int(counts[g])):
            px, py = (row % POOL_TILES_PER_ROW) * w, (row // POOL_TILES_PER_ROW) * h
            clean = c == 2                                       # every TU of every plane predicted exactly: every eob 0
            for t, (ox, oy) in enumerate(s.origins):
                for p in range(3):
                    size = TU if p == 0 else TU_UV
                    sx, sy, qx, qy = (x + ox, y + oy, px + ox, py + oy) if p == 0 else tuple(fu.round_uv(v) for v in (x + ox, y + oy, px + ox, py + oy))
                    blk = s.src[p][sy:sy + size, sx:sx + size].astype(np.int32)
                    exact = clean or (c + t + p + g) % 3 == 0    # this TU's prediction is the source
                    if not exact:
                        strength = 1 + (c + 2 * t + p) % 4
                        blk = blk + rng.normal(0, 4 * strength, blk.shape) + (9 + 6 * t) * (1 if (t + p) % 2 else -1)
                    s.pool[p][qy:qy + size, qx:qx + size] = np.clip(blk, 0, 255)
            inter = int(c % 2 == 0 or rng.random() < 0.4)
            f, d = fast[row], full[row]
            f["src_x"], f["src_y"], f["pred_x"], f["pred_y"], f["has_uv"] = x, y, px, py, 1
            f["flags"] = (mu.TYPE_INTER if inter else 0) | (mu.INVALID if c == 1 and g % 2 == 0 else 0)
            f["rate"], f["merge_rate"], f["lambda_"] = rng.integers(100, 9000), mu.NO_MERGE, rng.integers(500, 4000)
            d["luma_rate"], d["chroma_rate"] = rng.integers(50, 30000), rng.integers(10, 9000)
            d["skip_mode_rate"] = rng.integers(20, 3000) if inter and c % 4 != 3 else NONE
            d["lambda_"] = rng.integers(1000, 400000)
            d["recon_x"], d["recon_y"] = x, y
            d["qparam_index"] = 3 * int(rng.integers(0, len(fu.QINDICES))) + np.arange(3)
            d["tx_type_y"] = 0                                   # 64x64 has DCT_DCT alone
            d["tx_type_uv"] = BAD_UV_TYPE if c == 1 and g % 2 == 1 else types_uv[int(rng.integers(0, len(types_uv)))]
            d["txb_skip_ctx"], d["dc_sign_ctx"] = rng.integers(0, 13, 3), rng.integers(0, 3, 3)
            d["intra_mode"] = rng.integers(0, 13)
            row += 1
    if refuse:
        groups[n_groups // 2]["buffer_total_count"] = 0          # a group the pick refuses
    result = np.zeros(n_cand, mu.RESULT_DTYPE)
    result["cost"] = rng.integers(1000, 1 << 40, n_cand)
    s.fast, s.full, s.groups = fast, full, groups
    s.picks, s.pick_refused = mu.pick(result, fast, groups)
    assert s.pick_refused == refuse
    s.n_slots = n_groups * max_full
    slot_rows = (s.n_slots + SLOT_TILES_PER_ROW - 1) // SLOT_TILES_PER_ROW
    s.slot_shape = [(slot_rows * h, SLOT_TILES_PER_ROW * w)] + [(slot_rows * h // 2, SLOT_TILES_PER_ROW * w // 2)] * 2
    s.recon_shape = [p.shape for p in s.src]
    return s


def new_state(s):
    st = fu.new_state(s)
    st["tu"] = np.zeros(s.n_slots, TU_DTYPE)
    return st


def tile_xy(s, k):
    return (k % SLOT_TILES_PER_ROW) * s.tw, (k // SLOT_TILES_PER_ROW) * s.th


def _shift(v, shift):
    return v >> shift if shift >= 0 else (v << -shift) & U64


def full_loop(oracle, s, stages=LUMA | CHROMA | DECIDE, state=None):
    """svthip_md_full_loop128_batch_dev on scenario s; `state` carries what the device keeps in d_work, slot_recon and recon between calls.
    st["luma"][k] and st["chroma"][k] are lists over the TUs in the order of txb_itr."""
    sh = fu.shared()
    orc = fu._orc(oracle)
    st = state if state is not None else new_state(s)
    w, h, cw, ch = s.w, s.h, s.cw, s.ch
    origins = s.origins
    if stages & LUMA:
        for k in range(s.n_slots):
            g, i = divmod(k, s.max_full)
            n_full = fu.group_slots(s, g)
            row = fu.slot_row(s, g, i) if i < n_full else NONE
            use = row
            if use == NONE and n_full:
                use = fu.slot_row(s, g, 0)
            if use == NONE:
                use = 0
            if n_full == 0 and i == 0:
                st["refused"] += 1
            f, d = s.fast[use], s.full[use]
            inter = int(bool(f["flags"] & mu.TYPE_INTER))
            ty, tuv = int(d["tx_type_y"]), int(d["tx_type_uv"])      # used as given: no search from 128 on
            bad = not fu._type_valid(TU_UV, TU_UV, tuv) or not fu._type_valid(TU, TU, ty)
            if bad:
                ty = tuv = 0
                st["refused"] += row != NONE
            tx, ty_ = tile_xy(s, k)
            tus = []
            for ox, oy in origins:
                rec, q, eob, energy, d0, d1 = fu._chain(orc, sh, s.src[0], int(f["src_x"]) + ox, int(f["src_y"]) + oy, s.pool[0], int(f["pred_x"]) + ox,
                                                        int(f["pred_y"]) + oy, TU, TU, ty, int(d["qparam_index"][0]), TS_Y)
                st["slot"][0][ty_ + oy:ty_ + oy + TU, tx + ox:tx + ox + TU] = rec
                tus.append({"eob": eob, "energy": energy, "dist": (d0, d1), "bits": fu._bits(sh, q, eob, TS_Y, ty, 0, d, inter, s.reduced), "dc": int(q[0])})
            st["slots"][k] = {"row": row, "use": use, "tx_y": ty, "tx_uv": tuv, "bad": bad}
            st["luma"][k] = tus
    if stages & CHROMA:
        for k in range(s.n_slots):
            sl = st["slots"][k]
            f, d = s.fast[sl["use"]], s.full[sl["use"]]
            inter = int(bool(f["flags"] & mu.TYPE_INTER))
            tx, ty_ = tile_xy(s, k)
            tus = []
            for ox, oy in origins:
                sx, sy, px, py, qx, qy = (fu.round_uv(v) for v in (int(f["src_x"]) + ox, int(f["src_y"]) + oy, int(f["pred_x"]) + ox, int(f["pred_y"]) + oy,
                                                                   tx + ox, ty_ + oy))
                out = []
                for p in (1, 2):
                    rec, q, eob, _, d0, d1 = fu._chain(orc, sh, s.src[p], sx, sy, s.pool[p], px, py, TU_UV, TU_UV, sl["tx_uv"], int(d["qparam_index"][p]), TS_UV)
                    st["slot"][p][qy:qy + TU_UV, qx:qx + TU_UV] = rec
                    out.append({"eob": eob, "dist": (d0, d1), "bits": fu._bits(sh, q, eob, TS_UV, sl["tx_uv"], p, d, inter, s.reduced), "dc": int(q[0])})
                tus.append(out)
            st["chroma"][k] = tus
    if stages & DECIDE:
        shift_y, shift_uv = rate_util.tx_scale_shift(TS_Y), rate_util.tx_scale_shift(TS_UV)
        res, tu_rows = st["result"], st["tu"]
        res[:] = np.zeros(1, RESULT_DTYPE)[0]
        tu_rows[:] = np.zeros(1, TU_DTYPE)[0]
        for k in range(s.n_slots):
            sl, r = st["slots"][k], res[k]
            r["row"], r["tx_type_y"], r["tx_type_uv"], r["full_cost"] = sl["row"], sl["tx_y"], sl["tx_uv"], U64
            if sl["row"] == NONE:
                continue
            f, d = s.fast[sl["row"]], s.full[sl["row"]]
            if (f["flags"] & mu.INVALID) or sl["bad"]:
                continue
            lam = int(d["lambda_"])
            y, cb, cr, bits, masks, dcs = [0, 0], [0, 0], [0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]
            eobs = np.zeros((3, 4), np.uint16)
            for t, lu in enumerate(st["luma"][k]):              # ProductFullLoop's loop: the energy is the TU's own
                dist = [_shift(v + lu["energy"] & U64, shift_y) for v in lu["dist"]]
                t_bits, dist[0], _ = fu.tu_cost_luma(lam, lu["bits"], dist)
                y, bits[0] = [(y[0] + dist[0]) & U64, (y[1] + dist[1]) & U64], bits[0] + t_bits
                eobs[0, t], dcs[0] = lu["eob"], lu["dc"]         # quantized_dc[0] is overwritten by every TU
                masks[0] |= int(lu["eob"] != 0) << t
            if f["has_uv"]:
                for t, pair in enumerate(st["chroma"][k]):       # CuFullDistortionFastTuMode_R's loop
                    for p, dist in ((1, cb), (2, cr)):
                        c = pair[p - 1]
                        dist[:] = [(a + _shift(v, shift_uv)) & U64 for a, v in zip(dist, c["dist"])]
                        bits[p] += c["bits"]
                        eobs[p, t], dcs[p] = c["eob"], c["dc"]
                        masks[p] |= int(c["eob"] != 0) << t
            r["y_distortion"], r["cb_distortion"], r["cr_distortion"], r["coeff_bits"], r["quantized_dc"] = y, cb, cr, bits, dcs
            r["eob"] = eobs[:, 0]
            r["y_has_coeff"], r["u_has_coeff"], r["v_has_coeff"] = masks
            r["block_has_coeff"] = int(any(masks))
            tu_rows[k]["eob"] = eobs
            if int(d["skip_mode_rate"]) == NONE:
                r["full_cost"], r["full_lambda_rate"], r["full_cost_luma"] = fu.full_cost(lam, int(d["luma_rate"]), int(d["chroma_rate"]), y, cb, cr, bits)
            else:
                r["full_cost"], r["merge_cost"], r["skip_cost"], r["full_lambda_rate"], r["skip_flag"] = fu.merge_skip_cost(
                    lam, int(d["luma_rate"]), int(d["chroma_rate"]), int(d["skip_mode_rate"]), y, cb, cr, bits)
        dec = st["decision"]
        for g in range(s.n_groups):
            n_full = fu.group_slots(s, g)
            dec[g] = (U64, NONE, 0xFF, 0xFF, 0xFF, n_full)
            if n_full == 0:
                continue
            rows = res[g * s.max_full:g * s.max_full + n_full]
            intra = [int(r["row"]) != NONE and not (s.fast[int(r["row"])]["flags"] & mu.TYPE_INTER) for r in rows]
            modes = [int(s.full[int(r["row"])]["intra_mode"]) if int(r["row"]) != NONE else 0 for r in rows]
            win, best_intra = fu.mode_decision([int(c) for c in rows["full_cost"]], intra, modes)
            dec[g] = (rows[win]["full_cost"], rows[win]["row"], win, s.picks[g]["best"][win], best_intra, n_full)
            wrow = int(rows[win]["row"])
            if wrow == NONE:
                continue
            f, d = s.fast[wrow], s.full[wrow]
            tx, ty_ = tile_xy(s, g * s.max_full + win)
            rx, ry = int(d["recon_x"]), int(d["recon_y"])
            st["recon"][0][ry:ry + h, rx:rx + w] = st["slot"][0][ty_:ty_ + h, tx:tx + w]      # the whole slot tile: every TU of it
            if f["has_uv"]:
                for p in (1, 2):
                    st["recon"][p][fu.round_uv(ry):fu.round_uv(ry) + ch, fu.round_uv(rx):fu.round_uv(rx) + cw] = \
                        st["slot"][p][ty_ // 2:ty_ // 2 + ch, tx // 2:tx // 2 + cw]
    return st


def per_tu_numbers(s, st):
    """what the fixture keeps per (slot, TU): eob [3], bits [3], distortion sums before the shift [3][2], energy, first level [3]; rows of
    inactive slots repeat a valid candidate, as the launches do"""
    n_tu = len(s.origins)
    out = np.zeros((s.n_slots, n_tu, 16), np.int64)
    for k in range(s.n_slots):
        for t in range(n_tu):
            lu, ch = st["luma"][k][t], st["chroma"][k][t]
            planes = [lu] + ch
            out[k, t, 0:3] = [p["eob"] for p in planes]
            out[k, t, 3:6] = [p["bits"] for p in planes]
            out[k, t, 6:12] = [v for p in planes for v in p["dist"]]
            out[k, t, 12] = lu["energy"]
            out[k, t, 13:16] = [p["dc"] for p in planes]
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """the one-call result of a case, computed once and asserted equal to the fixture"""
    from oracle.binding import Oracle
    s = scenario(name)
    st = full_loop(Oracle(), s)
    fx = fixture()
    for key, got in (("result", st["result"]), ("tu", st["tu"]), ("decision", st["decision"]), ("per_tu", per_tu_numbers(s, st))):
        assert got.tobytes() == fx[f"{name}__{key}"].tobytes(), f"{name}: the restatement's {key} left the fixture"
    assert [fu.digest(st["slot"]), fu.digest(st["recon"])] == [str(v) for v in fx[f"{name}__digests"]] and st["refused"] == int(fx[f"{name}__refused"])
    return st


_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = dict(np.load(FIXTURE))
    return _FIXTURE


def coverage(s, st):
    """the conditions the fixture generator asserts of a case -> {name: bool}, from results alone (the restatement's or the reference's)"""
    res, full_mask = st["result"], (1 << len(s.origins)) - 1
    live = [k for k in range(s.n_slots) if int(res[k]["full_cost"]) != U64]
    rows = [st["slots"][k]["row"] for k in range(s.n_slots)]
    tu = st["tu"]["eob"]
    merge = [k for k in live if int(s.full[rows[k]]["skip_mode_rate"]) != NONE]
    return {
        "y mask partial": any(0 < int(res[k]["y_has_coeff"]) < full_mask for k in live),
        "uv mask partial": any(0 < int(res[k][n]) < full_mask for k in live for n in ("u_has_coeff", "v_has_coeff")),
        "every eob 0": any(not tu[k].any() for k in live),
        "dc of TU 0 differs from the last, Y": any(st["luma"][k][0]["dc"] != st["luma"][k][-1]["dc"] for k in live),
        "dc of TU 0 differs from the last, chroma": any(st["chroma"][k][0][p]["dc"] != st["chroma"][k][-1][p]["dc"] for k in live for p in (0, 1)),
        "three_quad_energy": any(lu["energy"] != 0 for k in live for lu in st["luma"][k]),
        "skip wins": any(int(res[k]["skip_flag"]) == 1 for k in merge),
        "merge wins": any(int(res[k]["skip_flag"]) == 0 for k in merge),
        "INVALID candidate": any(r != NONE and s.fast[r]["flags"] & mu.INVALID for r in rows),
        "refused group": any(fu.group_slots(s, g) == 0 for g in range(s.n_groups)),
        "tx_type_uv without a network": any(st["slots"][k]["bad"] and rows[k] != NONE for k in range(s.n_slots)),
    }


# ------------------------------------------------------------------------------------------------ the reference's own loops

TABLE_QINDEX_BUCKET = 1       # fu.shared()["tables"] is row 1 of tests/golden/coeff_rate.npz
CHROMA_DELTA_Q = -20          # the "inter" quantiser rows of tests/tq_util.py: av1_build_quantizer(8, 0, -20, -20, -20, -20)


def build_reference_driver(out_dir):
    import ctypes as C
    from oracle import ref_driver
    L = ref_driver.build_driver(os.path.join(ROOT, "tests", "golden", "ref_md_full128_driver.c"), out_dir)
    V = C.c_void_p
    L.drv_md_full128_init.argtypes = [C.c_int, C.c_int]
    L.drv_md_full128_geometry.argtypes = [C.c_int, C.c_int, V, V, V]
    L.drv_md_full128_full_loop.argtypes = [C.c_int, C.c_int, V, V, V, V, V, V, V, V, V]
    z = np.load(os.path.join(ROOT, "tests", "golden", "coeff_rate.npz"))
    assert L.drv_md_full128_init(int(z["qindices"][TABLE_QINDEX_BUCKET]), CHROMA_DELTA_Q) == 0
    return L


def reference_geometry(L, w, h):
    """(txb_count, [(tx_org_x, tx_org_y)], txsize, txsize_uv) of the reference's own BlockGeom"""
    n, org, ts = np.zeros(1, np.int32), np.zeros((4, 2), np.int32), np.zeros(2, np.int32)
    assert L.drv_md_full128_geometry(w, h, n.ctypes.data, org.ctypes.data, ts.ctypes.data) == 0
    return int(n[0]), [tuple(int(v) for v in o) for o in org[:int(n[0])]], int(ts[0]), int(ts[1])


def reference_slot(L, s, row):
    """ProductFullLoop, FullLoop_R, CuFullDistortionFastTuMode_R, the full cost and AV1PerformInverseTransformRecon of the reference on
    candidate `row` -> (out64 [15], out32 [19], [Y, Cb, Cr] reconstruction)"""
    import ctypes as C
    f, d = s.fast[row], s.full[row]
    qrows = [int(v) for v in d["qparam_index"]]
    assert qrows[1] == qrows[0] + 1 and qrows[2] == qrows[0] + 2 and qrows[0] % 3 == 0   # the reference has one qindex a picture
    inter, merge = int(bool(f["flags"] & mu.TYPE_INTER)), int(int(d["skip_mode_rate"]) != NONE)
    src, pred = [], []
    for p in range(3):
        sx, sy, px, py = (int(f[n]) if p == 0 else fu.round_uv(int(f[n])) for n in ("src_x", "src_y", "pred_x", "pred_y"))
        bw, bh = (s.w, s.h) if p == 0 else (s.cw, s.ch)
        src.append(np.ascontiguousarray(s.src[p][sy:sy + bh, sx:sx + bw]))
        pred.append(np.ascontiguousarray(s.pool[p][py:py + bh, px:px + bw]))
    ptrs = lambda a: (C.c_void_p * 3)(*[x.ctypes.data for x in a])  # noqa: E731
    strides = lambda a: np.array([x.strides[0] for x in a], np.int32)  # noqa: E731
    ss, ps = strides(src), strides(pred)
    args = np.array([fu.QINDICES[qrows[0] // 3], inter, merge, int(d["intra_mode"]), int(d["tx_type_y"]), int(d["tx_type_uv"]), *[int(v) for v in d["txb_skip_ctx"]],
                     *[int(v) for v in d["dc_sign_ctx"]], 0, s.reduced, int(d["skip_mode_rate"]) if merge else 0], np.int32)
    rates = np.array([int(d["luma_rate"]), int(d["chroma_rate"]), int(d["lambda_"])], np.uint64)
    out64, out32, recon = np.zeros(15, np.uint64), np.zeros(19, np.int32), np.zeros(s.w * s.h * 3 // 2, np.uint8)
    assert L.drv_md_full128_full_loop(s.w, s.h, ptrs(src), ss.ctypes.data, ptrs(pred), ps.ctypes.data, args.ctypes.data, rates.ctypes.data, out64.ctypes.data,
                              out32.ctypes.data, recon.ctypes.data) == 0
    ny, nc = s.w * s.h, s.cw * s.ch
    return out64, out32, [recon[:ny].reshape(s.h, s.w), recon[ny:ny + nc].reshape(s.ch, s.cw), recon[ny + nc:].reshape(s.ch, s.cw)]


def restated_slot(s, st, k):
    """slot k of a restated call in the layout of reference_slot"""
    r, n_tu = st["result"][k], len(s.origins)
    out64 = np.array([*r["y_distortion"], *r["cb_distortion"], *r["cr_distortion"], *r["coeff_bits"], r["full_cost"], r["merge_cost"], r["skip_cost"],
                      r["full_lambda_rate"], r["full_cost_luma"], st["luma"][k][n_tu - 1]["energy"]], np.uint64)
    out32 = np.array([*st["tu"][k]["eob"].reshape(-1), *r["quantized_dc"], r["y_has_coeff"], r["u_has_coeff"], r["v_has_coeff"], r["skip_flag"]], np.int32)
    tx, ty = tile_xy(s, k)
    tiles = [st["slot"][0][ty:ty + s.h, tx:tx + s.w]] + [st["slot"][p][ty // 2:ty // 2 + s.ch, tx // 2:tx // 2 + s.cw] for p in (1, 2)]
    return out64, out32, tiles


# ------------------------------------------------------------------------------------------------ the hand-over chain at 128x128

def chain_scenario():
    """two 128x128 blocks of a 256x128 picture with three inter candidates each (list 0, list 1, both), their prediction descriptors
    and the two references: what av1_inter_pred_batch_dev -> md_fast_cost_batch_dev -> md_fast_pick_batch_dev -> the full loop start from.
    A new object every call: the chain fills pool and picks."""
    import inter_pred_util as ipu
    w = h = 128
    rng = np.random.default_rng(128128)
    s = fu.Scenario()
    s.name, s.w, s.h, s.cw, s.ch, s.tw, s.th, s.n_groups, s.max_full, s.reduced = "chain128", w, h, 64, 64, w, h, 2, 3, 0
    s.origins = tu_origins(w, h)
    border = ipu.border_for(w, h)
    s.ref0, s.ref1 = (ipu.random_picture(rng, 256, 128, border, 8, "smooth") for _ in range(2))
    s.src = []
    for k, p in enumerate((s.ref0.y, s.ref0.cb, s.ref0.cr)):   # reference 0 moved by one sample, plus a little noise: residuals worth coding
        b, pw, ph = border >> (k > 0), 256 >> (k > 0), 128 >> (k > 0)
        s.src.append(np.clip(p[b + 1:b + 1 + ph, b + 1:b + 1 + pw].astype(np.int32) + rng.integers(-3, 4, (ph, pw)), 0, 255).astype(np.uint8))
    s.block_xy = [(0, 0), (128, 0)]
    s.n_cand = 6
    s.pu = ipu.random_descs(rng, 6, w, h, 256, 128, directions=(0, 1, 2, 0, 1, 2), clamp_frac=0.0, positions=[(0, 0)] * 3 + [(128, 0)] * 3)
    s.pu["mv"] = rng.integers(-20, 21, s.pu["mv"].shape)
    fast, full = np.zeros(6, fu.FAST_DTYPE), np.zeros(6, fu.FULL_DTYPE)
    s.pool = [np.full((2 * h, POOL_TILES_PER_ROW * w), 0x11, np.uint8)] + [np.full((h, POOL_TILES_PER_ROW * w // 2), 0x11, np.uint8) for _ in range(2)]
    types_uv = svtav1_hip.valid_tx_types(TU_UV, TU_UV)
    for row in range(6):
        x, y = s.block_xy[row // 3]
        px, py = (row % POOL_TILES_PER_ROW) * w, (row // POOL_TILES_PER_ROW) * h
        s.pu[row]["dst_origin_x"], s.pu[row]["dst_origin_y"] = px, py
        f, d = fast[row], full[row]
        f["src_x"], f["src_y"], f["pred_x"], f["pred_y"], f["has_uv"], f["flags"] = x, y, px, py, 1, mu.TYPE_INTER
        f["rate"], f["merge_rate"], f["lambda_"] = rng.integers(100, 9000), mu.NO_MERGE, rng.integers(500, 4000)
        d["luma_rate"], d["chroma_rate"] = rng.integers(50, 30000), rng.integers(10, 9000)
        d["skip_mode_rate"] = rng.integers(20, 3000) if row % 3 == 0 else NONE
        d["lambda_"] = rng.integers(1000, 400000)
        d["recon_x"], d["recon_y"] = x, y
        d["qparam_index"] = 3 * (row % len(fu.QINDICES)) + np.arange(3)
        d["tx_type_y"], d["tx_type_uv"] = 0, types_uv[row % len(types_uv)]
        d["txb_skip_ctx"], d["dc_sign_ctx"] = rng.integers(0, 13, 3), rng.integers(0, 3, 3)
    s.fast, s.full = fast, full
    s.groups = np.array([(0, 3, 2, 13), (3, 3, 3, 13)], fu.GROUP_DTYPE)   # two and three buffers: two and three slots
    s.picks = None
    s.n_slots = 6
    s.slot_shape = [(2 * h, SLOT_TILES_PER_ROW * w)] + [(h, SLOT_TILES_PER_ROW * w // 2)] * 2
    s.recon_shape = [p.shape for p in s.src]
    return s


def run_chain(oracle, s):
    """the restated chain on chain_scenario() -> {pool, fast, picks, state}"""
    import inter_pred_util as ipu
    pool = ipu.Picture(s.pool[0], s.pool[1], s.pool[2], 0)
    assert ipu.predict(s.ref0, s.ref1, pool, s.pu, s.w, s.h, 8) == 0
    fast = mu.fast_cost(s.src, s.pool, s.fast, s.w, s.h)
    s.picks, refused = mu.pick(fast, s.fast, s.groups)
    assert refused == 0
    return {"pool": [p.copy() for p in s.pool], "fast": fast, "picks": s.picks, "state": full_loop(oracle, s)}
