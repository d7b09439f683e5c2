"""numpy restatement of the coefficient rate (Av1TuEstimateCoeffBits / av1_cost_coeffs_txb) and of ProductFullLoopTxSearch's RD
decision, for the tests of svthip_coeff_rate_batch_dev and of the batcher's transform-type search.  Line numbers are those of the
reference (Source/Lib/Codec/...).  Each TU is vectorised over its coefficients: neighbour sums by array slicing, table gathers and
the mask iscan < eob."""
import ctypes as C
import os

import numpy as np

from oracle import ref_driver
from oracle.ref_driver import reference_available  # noqa: F401

# TxSize tables (EbDefinitions.h:1178-1219, EbTransforms.h:61-81, EbPictureControlSet.h:63)
TX_W = np.array([4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64])
TX_H = np.array([4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16])
SQR = np.array([0, 1, 2, 3, 4, 0, 0, 1, 1, 2, 2, 3, 3, 0, 0, 1, 1, 2, 2])
SQR_UP = np.array([0, 1, 2, 3, 4, 1, 1, 2, 2, 3, 3, 4, 4, 2, 2, 3, 3, 4, 4])
LOG2_MINUS4 = np.array([0, 2, 4, 6, 6, 1, 1, 3, 3, 5, 5, 6, 6, 2, 2, 4, 4, 5, 5])
# tx_type_to_class (EbCabacContextModel.h:818-835): 0 2-D, 1 horizontal, 2 vertical
TX_CLASS = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 1, 2, 1, 2, 1])
# EbDefinitions.h:1429-1479
NUM_EXT_TX_SET = [1, 2, 5, 7, 12, 16]
EXT_TX_SET_INDEX = [[0, -1, 2, 1, -1, -1], [0, 3, -1, -1, 2, 1]]
EXT_TX_USED = [0x0001, 0x0201, 0x020f, 0x0e0f, 0x0fff, 0xffff]
# allowed_tx_set_a (EbFullLoop.c:1095-1114) as masks, bit t = TxType t
ALLOWED_TX_SET_A = [0x0e0f, 0xae0f, 0x0e0f, 0x0201, 0x0001, 0x0e0f, 0x0e0f, 0xae0f, 0x5e0f, 0x0201, 0x0201, 0x0001, 0x0001, 0x0e0f,
                    0x0e0f, 0x0201, 0x0201, 0x0001, 0x0001]
EOB_GROUP_START = [0, 1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 513]   # k_eob_group_start (EbRateDistortionCost.c:195)
EOB_OFFSET_BITS = [0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9]             # k_eob_offset_bits
COST_LITERAL_1 = 512                                                 # av1_cost_literal(1), EbMdRateEstimation.h:25
MAX_CU_COST = (1 << 64) - 1 >> 1                                     # EbCodingUnit.h:39
U64 = (1 << 64) - 1


def ext_tx_set_type(tx_size, is_inter, reduced):
    """get_ext_tx_set_type (EbDefinitions.h:1442-1460)"""
    up, sq = SQR_UP[tx_size], SQR[tx_size]
    if up > 3:
        return 0
    if up == 3:
        return 1 if is_inter else 0
    if reduced:
        return 1 if is_inter else 2
    if is_inter:
        return 4 if sq == 2 else 5
    return 2 if sq == 2 else 3


def tx_search_type_mask(tx_size, is_inter, reduced, fast):
    """ProductFullLoopTxSearch's candidates (EbFullLoop.c:1160-1197): av1_ext_tx_used of the set, DCT_DCT only above 32x32, DCT_DCT
    if nothing is left; with the fast search (ENC_M1) only the types of allowed_tx_set_a are visited"""
    m = EXT_TX_USED[ext_tx_set_type(tx_size, is_inter, reduced)]
    if SQR_UP[tx_size] > 3:
        m &= 1
    if not m:
        m = 1
    if fast:
        m &= ALLOWED_TX_SET_A[tx_size]
    return m


def tx_type_bits(tables, tx_size, tx_type, is_inter, intra_mode, reduced):
    """Av1TransformTypeRateEstimation (EbRateDistortionCost.c:154-193), luma"""
    st = ext_tx_set_type(tx_size, is_inter, reduced)
    if NUM_EXT_TX_SET[st] <= 1:
        return 0
    s = EXT_TX_SET_INDEX[1 if is_inter else 0][st]
    if s <= 0:
        return 0
    if is_inter:
        return int(tables["interTxTypeFacBits"][s, SQR[tx_size], tx_type])
    return int(tables["intraTxTypeFacBits"][s, SQR[tx_size], intra_mode, tx_type])


def eob_cost(eob, eob_costs, cc, tx_class):
    """get_eob_cost (:228-244) with get_eob_pos_token (:210-226)"""
    if eob < 33:
        pt = [0, 1, 2, 3, 3, 4, 4, 4, 4][eob] if eob <= 8 else (5 if eob <= 16 else 6)
    else:
        e = min((eob - 1) >> 5, 16)
        pt = 7 if e <= 1 else 8 if e <= 3 else 9 if e <= 7 else 10 if e <= 15 else 11
    extra = eob - EOB_GROUP_START[pt]
    cost = int(eob_costs[0 if tx_class == 0 else 1, pt - 1])
    ob = EOB_OFFSET_BITS[pt]
    if ob > 0:
        cost += int(cc["eob_extra_cost"][pt, (extra >> (ob - 1)) & 1])
        if ob > 1:
            cost += COST_LITERAL_1 * (ob - 1)
    return cost


def _nz_offsets(tx_size, tx_class, Ha, Wa):
    """position offsets of av1_get_nz_map_contexts_sse2 (ASM_SSE2/encodetxb_sse2.c:92-455): 2-D by the REAL shape"""
    r, c = np.mgrid[0:Ha, 0:Wa]
    if tx_class == 1:
        return 26 + np.where(c == 0, 0, np.where(c == 1, 5, 10))
    if tx_class == 2:
        return 26 + np.where(r == 0, 0, np.where(r == 1, 5, 10))
    W, H = TX_W[tx_size], TX_H[tx_size]
    rc = r + c
    near = np.where(rc <= 3, 6, 21)
    if W == H:
        off = np.where(rc == 1, 1, near)
    elif W > H:
        off = np.where(c < 2, 16, near)
    else:
        off = np.where(r < 2, 11, near)
    off[0, 0] = 0
    return off


def coeff_bits(tables, levels, iscan, eob, tx_size, tx_type, plane_type=0, txb_skip_ctx=0, dc_sign_ctx=0, is_inter=1, intra_mode=0,
               reduced_tx_set=0):
    """Av1TuEstimateCoeffBits for one plane (EbRateDistortionCost.c:1350-1460).  levels / iscan: min(W,32) x min(H,32), raster."""
    txs_ctx = (SQR[tx_size] + SQR_UP[tx_size] + 1) >> 1
    cc = tables["coeffFacBits"][txs_ctx, plane_type]
    if eob == 0:
        return int(cc["txb_skip_cost"][txb_skip_ctx, 1])                     # av1_cost_skip_txb (:485-493)
    Wa, Ha = min(TX_W[tx_size], 32), min(TX_H[tx_size], 32)
    n = Wa * Ha
    tx_class = TX_CLASS[tx_type]
    q = np.asarray(levels, np.int64).reshape(Ha, Wa)
    si = np.asarray(iscan, np.int64).reshape(Ha, Wa)
    lvl = np.abs(q)
    P = np.zeros((Ha + 4, Wa + 4), np.int64)                                 # av1_txb_init_levels_c (:124-145), TX_PAD_HOR / _BOTTOM
    P[:Ha, :Wa] = np.minimum(lvl, 127)
    m3 = np.minimum(P, 3)
    cost = int(cc["txb_skip_cost"][txb_skip_ctx, 0])
    if plane_type == 0:
        cost += tx_type_bits(tables, tx_size, tx_type, is_inter, intra_mode, reduced_tx_set)
    cost += eob_cost(eob, tables["eobFracBits"][LOG2_MINUS4[tx_size], plane_type], cc, tx_class)
    # nz-map contexts (get_nz_mag :378-404 / the SSE2 kernel's five neighbours)
    s = m3[0:Ha, 1:Wa + 1] + m3[1:Ha + 1, 0:Wa]
    if tx_class == 0:
        s = s + m3[1:Ha + 1, 1:Wa + 1] + m3[0:Ha, 2:Wa + 2] + m3[2:Ha + 2, 0:Wa]
    elif tx_class == 1:
        s = s + m3[0:Ha, 2:Wa + 2] + m3[0:Ha, 3:Wa + 3] + m3[0:Ha, 4:Wa + 4]
    else:
        s = s + m3[2:Ha + 2, 0:Wa] + m3[3:Ha + 3, 0:Wa] + m3[4:Ha + 4, 0:Wa]
    ctx = np.minimum((s + 1) >> 1, 4)
    if tx_class == 0:
        ctx[0, 0] = 0
    ctx = ctx + _nz_offsets(tx_size, tx_class, Ha, Wa)
    inside = si < eob
    last = si == eob - 1
    last_ctx = 0 if eob == 1 else (1 if eob - 1 <= n // 8 else 2 if eob - 1 <= n // 4 else 3)    # encodetxb_sse2.c:548-555
    l3 = np.minimum(lvl, 3)
    base = np.where(last, cc["base_eob_cost"][last_ctx, np.maximum(l3 - 1, 0)], cc["base_cost"][ctx, l3])
    total = cost + int(base[inside].sum())
    nz = inside & (lvl > 0)
    sign = np.where(si == 0, cc["dc_sign_cost"][dc_sign_ctx, (q < 0).astype(np.int64)], COST_LITERAL_1)
    total += int(sign[nz].sum())
    # get_br_ctx (:454-483) and lps_cost, get_golomb_cost (:97-103) on the true level
    mag = P[0:Ha, 1:Wa + 1] + P[1:Ha + 1, 0:Wa]
    if tx_class == 0:
        mag = mag + P[1:Ha + 1, 1:Wa + 1]
    elif tx_class == 1:
        mag = mag + P[0:Ha, 2:Wa + 2]
    else:
        mag = mag + P[2:Ha + 2, 0:Wa]
    br = np.minimum((mag + 1) >> 1, 6)
    r, c = np.mgrid[0:Ha, 0:Wa]
    near = (r < 2) & (c < 2) if tx_class == 0 else (c == 0 if tx_class == 1 else r == 0)
    br = np.where((r == 0) & (c == 0), br, np.where(near, br + 7, br + 14))
    hi = nz & (lvl > 2)
    lps = cc["lps_cost"][br, np.minimum(np.maximum(lvl - 3, 0), 12)]
    total += int(lps[hi].sum())
    g = hi & (lvl >= 15)
    if g.any():
        length = np.array([int(v - 14).bit_length() for v in lvl[g]])
        total += int((COST_LITERAL_1 * (2 * length - 1)).sum())
    return total


def tx_scale_shift(tx_size):
    """(MAX_TX_SCALE - av1_get_tx_scale(tx_size)) * 2 (EbFullLoop.c:1281, EbTransforms.h:312-316)"""
    pels = int(TX_W[tx_size] * TX_H[tx_size])
    return (1 - ((pels > 256) + (pels > 1024))) * 2


def decide(tx_size, lam, cands):
    """ProductFullLoopTxSearch's loop (EbFullLoop.c:1198-1342, TX_TYPE_FIX, BUG_FIX, CBF_ZERO_OFF).  cands: {tx_type: (eob, energy,
    dist_residual, dist_prediction, bits)}; visited in ascending type order.  Returns the winner as a dict."""
    shift = tx_scale_shift(tx_size)
    best_cost = U64
    cur = {"full_cost": MAX_CU_COST, "coeff_bits": 0, "distortion": (0, 0), "eob": 0}   # yFullCost's initial value, and nothing else
    best = None
    for tt in sorted(cands):
        eob, energy, d0, d1, bits = (int(v) for v in cands[tt])
        if eob != 0 or tt == 0:         # :1248-1253: eob == 0 and not DCT_DCT -> continue, yFullCost stays as it was
            d0, d1 = (d0 + energy) & U64, (d1 + energy) & U64
            d0, d1 = ((d0 << -shift) & U64, (d1 << -shift) & U64) if shift < 0 else (d0 >> shift, d1 >> shift)
            nz_cost = (((bits * lam) & U64) + 256 >> 9) + ((d0 << 7) & U64) & U64     # RDCOST (EbRateDistortionCost.h:215-217)
            nz = nz_cost < U64                                                     # Av1TuCalcCostLuma :2208-2227, CBF_ZERO_OFF
            cur = {"full_cost": nz_cost, "coeff_bits": bits if nz else 0, "distortion": (d0 if nz else d1, d1), "eob": eob}
        if cur["full_cost"] < best_cost:
            best_cost = cur["full_cost"]
            best = dict(cur, tx_type=tt)
    return best


# ---------------------------------------------------------------------------------------------------------------------
# the reference driver (tests/golden/ref_coeff_rate_driver.c), built where the reference and the oracle's objects exist
# ---------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_reference_driver(out_dir):
    """The driver by the recipe of oracle/ref_driver.py, with its signatures."""
    L = ref_driver.build_driver(os.path.join(ROOT, "tests", "golden", "ref_coeff_rate_driver.c"), out_dir)
    L.drv_init.restype = C.c_int
    L.drv_init.argtypes = [C.c_int]
    L.drv_tables.restype = None
    L.drv_tables.argtypes = [C.c_void_p]
    L.drv_bits.restype = C.c_uint64
    L.drv_bits.argtypes = [C.c_void_p, C.c_uint32] + [C.c_int] * 8
    for fn in ("drv_ext_tx_set_type", "drv_ext_tx_used", "drv_allowed_tx_set_a", "drv_txsize_sqr_up"):
        getattr(L, fn).restype = C.c_int
    return L


def reference_tables(L, base_qindex, dtype):
    assert L.drv_init(base_qindex) == 0
    t = np.zeros(1, dtype)
    L.drv_tables(t.ctypes.data)
    return t


def reference_mask(L, tx_size, is_inter, reduced, fast):
    """the candidate mask of EbFullLoop.c:1160-1197, from the reference's own tables"""
    st = L.drv_ext_tx_set_type(tx_size, int(is_inter), int(reduced))
    m = 0
    for t in range(16):
        ref_t = 0 if (not L.drv_ext_tx_used(st, t) or L.drv_txsize_sqr_up(tx_size) > 3) else t
        if ref_t == t:
            m |= 1 << t
    if not m:
        m = 1
    if fast:
        m &= sum(1 << t for t in range(16) if L.drv_allowed_tx_set_a(tx_size, t))
    return m
