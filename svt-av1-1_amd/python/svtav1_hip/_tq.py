"""Transform, quantisation and reconstruction of transform units (include/svtav1_hip.h: the batched stages, the fused encode chain,
the batching layer, coefficient rate and the RD transform-type search)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._core import _check, lib

QUANT_DESC_DTYPE = _abi.dtype("svthip_quant_desc")

TXFM_DESC_DTYPE = _abi.dtype("svthip_txfm_desc")
ITXFM_DESC_DTYPE = _abi.dtype("svthip_itxfm_desc")
TU_DESC_DTYPE = _abi.dtype("svthip_tu_desc")

# the 19 AV1 transform sizes (width, height), TxSize order (Codec/EbDefinitions.h)
TX_SIZES_WH = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (4, 8), (8, 4), (8, 16), (16, 8), (16, 32), (32, 16), (32, 64),
               (64, 32), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]
_VTX = [0, 1, 0, 1, 2, 0, 2, 1, 2, 3, 0, 3, 1, 3, 2, 3]  # vtx_tab / htx_tab (Codec/EbTransforms.h:88-97): 0 DCT 1 ADST 2 FLIPADST 3 IDTX
_HTX = [0, 0, 1, 1, 0, 2, 2, 2, 1, 3, 3, 0, 3, 1, 3, 2]


def valid_tx_types(w: int, h: int):
    """TxTypes for which the reference has 1-D networks at this size (ADST up to 16 points, identity up to 32, 64 DCT only)."""
    out = []
    for t in range(16):
        kc, kr = _VTX[t], _HTX[t]
        if (kc in (1, 2) and h > 16) or (kr in (1, 2) and w > 16) or (kc == 3 and h > 32) or (kr == 3 and w > 32):
            continue
        out.append(t)
    return out


TuResult = _abi.structure("svthip_tu_result")
TU_RECON_SCRATCH = _abi.define("SVTHIP_TU_RECON_SCRATCH")


class TuBatcher:
    """svthip_tu_batcher: host-side gather / scatter of (TU, tx_type) candidates for the fused T/Q chain."""

    def __init__(self, ctx: "Context", max_candidates: int, max_coeff_samples: int):
        self._h = C.c_void_p()
        self._ctx = ctx
        _check(lib().svthip_tu_batcher_create(ctx._h, max_candidates, max_coeff_samples, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().svthip_tu_batcher_destroy(self._h)
            self._h = C.c_void_p()

    def begin(self, d_src, d_pred, d_recon, planes_16bit, d_qparams, d_iscan):
        _check(lib().svthip_tu_batcher_begin(self._h, d_src, d_pred, d_recon, int(planes_16bit), d_qparams, d_iscan))

    def add(self, tx_size, tx_type, src_offset, src_stride, pred_offset, pred_stride, recon_offset, recon_stride, qparam_index, iscan_offset) -> int:
        h = C.c_uint32(0)
        _check(lib().svthip_tu_batcher_add(self._h, tx_size, tx_type, src_offset, src_stride, pred_offset, pred_stride, recon_offset, recon_stride,
                                           qparam_index, iscan_offset, C.byref(h)))
        return h.value

    def flush(self):
        _check(lib().svthip_tu_batcher_flush(self._h))

    def result(self, handle) -> TuResult:
        r = TuResult()
        _check(lib().svthip_tu_batcher_result(self._h, handle, C.byref(r)))
        return r

    def read_coeffs(self, handle, n):
        q = np.zeros(n, np.int32); dq = np.zeros(n, np.int32)
        _check(lib().svthip_tu_batcher_read_coeffs(self._h, handle, q.ctypes.data, dq.ctypes.data))
        return q, dq

    def pools(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().svthip_tu_batcher_pools(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_tx_search(self, d_tables, iscan_offsets):
        """d_tables: device address of a COEFF_RATE_TABLES_DTYPE record; iscan_offsets: [19][16] (or 304) iscan-pool offsets"""
        off = np.ascontiguousarray(np.asarray(iscan_offsets, np.uint32).reshape(19 * 16))
        _check(lib().svthip_tu_batcher_set_tx_search(self._h, d_tables, off.ctypes.data))

    def add_tx_search(self, tu: "TxSearchTu" = None, **fields) -> int:
        """one TU of the RD transform-type search (a TxSearchTu, or its fields as keywords); returns the TU handle"""
        if tu is None:
            tu = TxSearchTu(**fields)
        h = C.c_uint32(0)
        _check(lib().svthip_tu_batcher_add_tx_search(self._h, C.byref(tu), C.byref(h)))
        return h.value

    def tx_search_result(self, tu_handle) -> "TxSearchResult":
        r = TxSearchResult()
        _check(lib().svthip_tu_batcher_tx_search_result(self._h, tu_handle, C.byref(r)))
        return r


# ---- coefficient rate and the RD transform-type search (include/svtav1_hip.h) ----
LV_MAP_COEFF_COST_DTYPE = _abi.dtype("svthip_lv_map_coeff_cost")
# svthip_coeff_rate_tables; hand-written: the recorded form gives eobFracBits, [7][2] of svthip_lv_map_eob_cost { eob_cost[2][11] }, as one array
COEFF_RATE_TABLES_DTYPE = np.dtype([("coeffFacBits", LV_MAP_COEFF_COST_DTYPE, (5, 2)), ("eobFracBits", "<i4", (7, 2, 2, 11)),
                                    ("interTxTypeFacBits", "<i4", (4, 4, 17)), ("intraTxTypeFacBits", "<i4", (3, 4, 13, 17))])
COEFF_RATE_DESC_DTYPE = _abi.dtype("svthip_coeff_rate_desc")
TxSearchTu = _abi.structure("svthip_tx_search_tu", lambda_="lambda")
TxSearchResult = _abi.structure("svthip_tx_search_result")


def tx_search_type_mask(tx_size: int, is_inter: bool, reduced_tx_set: bool, fast_tx_search: bool) -> int:
    """the reference's transform-type candidate mask of ProductFullLoopTxSearch (bit t = TxType t)"""
    return int(lib().svthip_tx_search_type_mask(tx_size, int(bool(is_inter)), int(bool(reduced_tx_set)), int(bool(fast_tx_search))))


class TransformQuant:
    """the batched transform / quantisation entries as Context methods"""

    def quantize_b_batch_dev(self, d_coeff, d_desc, n_tu, d_qparams, d_iscan, d_qcoeff, d_dqcoeff, d_eob, stream=None):
        _check(lib().svthip_quantize_b_batch_dev(self._h, d_coeff, d_desc, n_tu, d_qparams, d_iscan, d_qcoeff, d_dqcoeff, d_eob, stream))

    def fwd_txfm2d_batch_dev(self, d_residual, d_desc, n_tu, tx_width, tx_height, bit_depth, d_coeff, stream=None):
        _check(lib().svthip_fwd_txfm2d_batch_dev(self._h, d_residual, d_desc, n_tu, tx_width, tx_height, bit_depth, d_coeff, stream))

    def inv_txfm2d_add_batch_dev(self, d_coeff, d_desc, n_tu, tx_width, tx_height, bit_depth, recon_16bit, d_recon, stream=None):
        _check(lib().svthip_inv_txfm2d_add_batch_dev(self._h, d_coeff, d_desc, n_tu, tx_width, tx_height, bit_depth, int(recon_16bit),
                                                     d_recon, stream))

    def encode_tu_batch_dev(self, d_src, d_pred, d_recon, d_desc, n_tu, tx_width, tx_height, d_qparams, d_iscan, d_coeff, d_qcoeff,
                            d_dqcoeff, d_eob, d_energy=None, d_dist=None, stream=None, planes_16bit=False):
        fn = lib().svthip_encode_tu16_batch_dev if planes_16bit else lib().svthip_encode_tu_batch_dev
        _check(fn(self._h, d_src, d_pred, d_recon, d_desc, n_tu, tx_width, tx_height, d_qparams, d_iscan,
                  d_coeff, d_qcoeff, d_dqcoeff, d_eob, d_energy, d_dist, stream))

    def coeff_rate_batch_dev(self, d_tables, d_qcoeff, d_eob, d_iscan, d_desc, n_tu, tx_size, d_bits, stream=None):
        """Av1TuEstimateCoeffBits of n_tu TUs of one TxSize (COEFF_RATE_DESC_DTYPE descriptors, uint16 eobs) -> uint32 bits per TU"""
        _check(lib().svthip_coeff_rate_batch_dev(self._h, d_tables, d_qcoeff, d_eob, d_iscan, d_desc, n_tu, tx_size, d_bits, stream))
