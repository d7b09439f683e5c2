"""Prediction (include/svtav1_hip.h): luma convolutions, whole-PU inter prediction, warped motion, intra prediction."""
from __future__ import annotations

import ctypes as C

from . import _abi
from ._core import _check, lib

CONVOLVE_DESC_DTYPE = _abi.dtype("svthip_convolve_desc")
# the 22 AV1 block sizes (width, height)
AV1_BLOCK_SIZES_WH = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64),
                      (64, 128), (128, 64), (128, 128), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]

CONVOLVE_COMPOUND_DESC_DTYPE = _abi.dtype("svthip_convolve_compound_desc")

# ---- whole-PU inter prediction (svthip_av1_inter_pred_batch_dev / svthip_av1_highbd_inter_pred_batch_dev) ----
INTER_PU_DESC_DTYPE = _abi.dtype("svthip_inter_pu_desc")
UNI_PRED_LIST_0, UNI_PRED_LIST_1, BI_PRED = 0, 1, 2
# svthip_inter_planes: device pointers at picture sample (0, 0) of Y / Cb / Cr, strides in samples (Cb and Cr share c_stride).
InterPlanes = _abi.structure("svthip_inter_planes")


def _planes_arg(p):
    return None if p is None else C.byref(p)


# ---- warped-motion prediction of whole PUs (svthip_av1_warped_pred_batch_dev / svthip_av1_highbd_warped_pred_batch_dev) ----
WARP_PU_DESC_DTYPE = _abi.dtype("svthip_warp_pu_desc")
WARP_ROTZOOM, WARP_AFFINE = 2, 3
WARP_BLOCK_SIZES_WH = [s for s in AV1_BLOCK_SIZES_WH if min(s) >= 8]

# ---- intra prediction of transform blocks (svthip_av1_intra_pred_batch_dev / svthip_av1_highbd_intra_pred_batch_dev) ----
INTRA_DESC_DTYPE = _abi.dtype("svthip_intra_desc")


class Prediction:
    """the prediction entries as Context methods"""

    def av1_convolve_sr_batch_dev(self, d_src, src_stride, d_dst, dst_stride, d_desc, n_blocks, width, height, stream=None):
        """8-bit single-reference AV1 convolution (2-D / x / y / copy by phase) of n_blocks blocks of one size."""
        _check(lib().svthip_av1_convolve_sr_batch_dev(self._h, d_src, src_stride, d_dst, dst_stride, d_desc, n_blocks, width, height, stream))

    def av1_convolve_compound_batch_dev(self, d_src0, src0_stride, d_src1, src1_stride, d_dst, dst_stride, d_desc, n_blocks, width, height, stream=None):
        """BI_PRED luma prediction of n_blocks blocks of one size (CONVOLVE_COMPOUND_DESC_DTYPE descriptors; subpel = x | y << 4)."""
        _check(lib().svthip_av1_convolve_compound_batch_dev(self._h, d_src0, src0_stride, d_src1, src1_stride, d_dst, dst_stride, d_desc, n_blocks, width,
                                                            height, stream))

    def av1_highbd_convolve_batch_dev(self, d_src0, src0_stride, d_src1, src1_stride, d_dst, dst_stride, d_desc, compound, n_blocks, width, height,
                                      bit_depth=10, stream=None):
        """10-bit inter prediction in 16-bit planes (offsets / strides in samples); compound selects the descriptor type."""
        _check(lib().svthip_av1_highbd_convolve_batch_dev(self._h, d_src0, src0_stride, d_src1, src1_stride, d_dst, dst_stride, d_desc, int(compound),
                                                          n_blocks, width, height, bit_depth, stream))

    def av1_inter_pred_batch_dev(self, ref0, ref1, dst, d_desc, n_pu, bwidth, bheight, stream=None):
        """8-bit whole-PU inter prediction (Y, Cb, Cr) of n_pu PUs of one luma size; ref0 / ref1 / dst are InterPlanes, d_desc a device
        array of INTER_PU_DESC_DTYPE."""
        _check(lib().svthip_av1_inter_pred_batch_dev(self._h, _planes_arg(ref0), _planes_arg(ref1), _planes_arg(dst), d_desc, n_pu, bwidth, bheight,
                                                     stream))

    def av1_highbd_inter_pred_batch_dev(self, ref0, ref1, dst, d_desc, n_pu, bwidth, bheight, bit_depth=10, stream=None):
        """The same for 16-bit planes holding 10-bit samples."""
        _check(lib().svthip_av1_highbd_inter_pred_batch_dev(self._h, _planes_arg(ref0), _planes_arg(ref1), _planes_arg(dst), d_desc, n_pu, bwidth,
                                                            bheight, bit_depth, stream))

    def inter_pred_refused(self):
        """Synchronises with the last inter-prediction call; raises SvtHipError naming the count if the device refused PUs since the last query."""
        n = C.c_uint32(0)
        _check(lib().svthip_inter_pred_refused(self._h, C.byref(n)))
        return n.value

    def av1_warped_pred_batch_dev(self, ref, dst, pic_width, pic_height, d_desc, n_pu, bwidth, bheight, stream=None):
        """8-bit warped-motion prediction (Y, Cb, Cr) of n_pu PUs of one luma size; ref / dst are InterPlanes, d_desc a device array of
        WARP_PU_DESC_DTYPE, pic_width x pic_height the reference picture's size (the warp clamps its reads to it)."""
        _check(lib().svthip_av1_warped_pred_batch_dev(self._h, _planes_arg(ref), _planes_arg(dst), pic_width, pic_height, d_desc, n_pu, bwidth,
                                                      bheight, stream))

    def av1_highbd_warped_pred_batch_dev(self, ref, dst, pic_width, pic_height, d_desc, n_pu, bwidth, bheight, bit_depth=10, stream=None):
        """The same for 16-bit planes holding 10-bit samples."""
        _check(lib().svthip_av1_highbd_warped_pred_batch_dev(self._h, _planes_arg(ref), _planes_arg(dst), pic_width, pic_height, d_desc, n_pu,
                                                             bwidth, bheight, bit_depth, stream))

    def av1_intra_pred_batch_dev(self, d_edge, d_dst, d_desc, n_blocks, tx_size, d_src=None, d_sad=None, stream=None):
        """8-bit intra prediction of n_blocks transform blocks of one TxSize; d_desc a device array of INTRA_DESC_DTYPE, d_edge the samples
        the edges are read from, d_dst where the blocks go (may be d_edge); d_sad (uint32 per block) asks for the SAD against d_src."""
        _check(lib().svthip_av1_intra_pred_batch_dev(self._h, d_edge, d_dst, d_desc, n_blocks, tx_size, d_src, d_sad, stream))

    def av1_highbd_intra_pred_batch_dev(self, d_edge, d_dst, d_desc, n_blocks, tx_size, bit_depth=10, stream=None):
        """The same for 16-bit samples holding 10-bit values (no SAD)."""
        _check(lib().svthip_av1_highbd_intra_pred_batch_dev(self._h, d_edge, d_dst, d_desc, n_blocks, tx_size, bit_depth, stream))
