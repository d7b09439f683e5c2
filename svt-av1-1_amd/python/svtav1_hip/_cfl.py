"""Chroma-from-luma prediction and its alpha search (svthip_av1_[highbd_]cfl_pred_batch_dev, svthip_av1_cfl_alpha_candidates_batch_dev,
svthip_cfl_alpha_decision_batch_dev)."""
from __future__ import annotations

from . import _abi
from ._core import _check, lib

CFL_DESC_DTYPE = _abi.dtype("svthip_cfl_desc")
CFL_DECISION_JOB_DTYPE = _abi.dtype("svthip_cfl_decision_job")   # `lambda` keeps its C spelling here
CFL_DECISION_DTYPE = _abi.dtype("svthip_cfl_decision")
# the luma sizes the reference uses CfL with
CFL_LUMA_SIZES_WH = [(8, 8), (16, 8), (8, 16), (16, 16), (32, 8), (8, 32), (32, 16), (16, 32), (32, 32)]


class Cfl:
    """the chroma-from-luma entries as Context methods"""

    def av1_cfl_pred_batch_dev(self, d_luma, d_cb, d_cr, d_cb_dst, d_cr_dst, d_desc, n_blocks, luma_w, luma_h, stream=None):
        """8-bit CfL prediction of n_blocks blocks of one luma size over the DC prediction in d_cb / d_cr; d_desc a device array of
        CFL_DESC_DTYPE; d_cb_dst / d_cr_dst may be d_cb / d_cr."""
        _check(lib().svthip_av1_cfl_pred_batch_dev(self._h, d_luma, d_cb, d_cr, d_cb_dst, d_cr_dst, d_desc, n_blocks, luma_w, luma_h, stream))

    def av1_highbd_cfl_pred_batch_dev(self, d_luma, d_cb, d_cr, d_cb_dst, d_cr_dst, d_desc, n_blocks, luma_w, luma_h, bit_depth=10, stream=None):
        """The same for 16-bit samples holding 10-bit values."""
        _check(lib().svthip_av1_highbd_cfl_pred_batch_dev(self._h, d_luma, d_cb, d_cr, d_cb_dst, d_cr_dst, d_desc, n_blocks, luma_w, luma_h, bit_depth,
                                                          stream))

    def av1_cfl_alpha_candidates_batch_dev(self, d_luma, d_cb_dc, d_cr_dc, d_desc, n_blocks, luma_w, luma_h, d_candidates, stream=None):
        """The 2 x 33 candidate tiles per block (alpha_q3 = -16 .. 16 on Cb, then on Cr) into the pool d_candidates."""
        _check(lib().svthip_av1_cfl_alpha_candidates_batch_dev(self._h, d_luma, d_cb_dc, d_cr_dc, d_desc, n_blocks, luma_w, luma_h, d_candidates, stream))

    def cfl_alpha_decision_batch_dev(self, d_distortion, d_bits, dist_shift, d_alpha_bits, d_job, n_blocks, d_out, stream=None):
        """cfl_rd_pick_alpha's walk over the candidates' costs: d_job of CFL_DECISION_JOB_DTYPE, d_out of CFL_DECISION_DTYPE."""
        _check(lib().svthip_cfl_alpha_decision_batch_dev(self._h, d_distortion, d_bits, dist_shift, d_alpha_bits, d_job, n_blocks, d_out, stream))
