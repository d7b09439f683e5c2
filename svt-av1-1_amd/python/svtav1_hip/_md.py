"""Mode decision's fast loop (svthip_md_fast_cost_batch_dev, svthip_md_fast_pick_batch_dev): pointer marshalling only.

The four structs cross Python as numpy arrays in device memory; md_fast_desc_dtype() / md_fast_result_dtype() / md_fast_group_dtype() /
md_fast_pick_dtype() give their layouts (svthip_md_fast_desc, _result, _group, _pick of include/svtav1_hip.h)."""
from __future__ import annotations

import numpy as np

from ._core import _check, lib
from ._pred import _planes_arg

MD_FAST_LUMA_GIVEN, MD_FAST_SKIP_DISTORTION, MD_FAST_INVALID, MD_FAST_CHROMA_QUARTER, MD_FAST_TYPE_INTER = 1, 2, 4, 8, 16
MD_FAST_MAX_CANDIDATES, MD_FAST_MAX_BUFFERS = 113, 13


def md_fast_desc_dtype() -> np.dtype:
    """svthip_md_fast_desc, 32 bytes; `lambda` is spelled lambda_"""
    return np.dtype([("src_x", "<u2"), ("src_y", "<u2"), ("pred_x", "<u2"), ("pred_y", "<u2"), ("rate", "<u4"), ("merge_rate", "<u4"),
                     ("lambda_", "<u4"), ("luma_given", "<u4"), ("has_uv", "u1"), ("flags", "u1"), ("reserved", "u1", (6,))])


def md_fast_result_dtype() -> np.dtype:
    """svthip_md_fast_result, 16 bytes"""
    return np.dtype([("luma", "<u4"), ("chroma", "<u4"), ("cost", "<u8")])


def md_fast_group_dtype() -> np.dtype:
    """svthip_md_fast_group, 8 bytes"""
    return np.dtype([("first", "<u4"), ("count", "<u2"), ("buffer_total_count", "u1"), ("buffer_width", "u1")])


def md_fast_pick_dtype() -> np.dtype:
    """svthip_md_fast_pick, 32 bytes"""
    return np.dtype([("best", "u1", (13,)), ("buffer_cand", "u1", (13,)), ("full_count", "u1"), ("disable_merge_index", "u1"),
                     ("reserved", "u1", (4,))])


class ModeDecisionFast:
    """the fast-loop entries as Context methods; src / pred are InterPlanes of 8-bit planes, the arrays device pointers"""

    def md_fast_cost_batch_dev(self, src, pred, d_desc, n_cand, bwidth, bheight, d_result, stream=None):
        """luma and chroma SAD and the fast cost of n_cand predicted PUs of one luma size: d_desc an array of md_fast_desc_dtype(),
        d_result one of md_fast_result_dtype()"""
        _check(lib().svthip_md_fast_cost_batch_dev(self._h, _planes_arg(src), _planes_arg(pred), d_desc, n_cand, bwidth, bheight, d_result, stream))

    def md_fast_pick_batch_dev(self, d_result, d_desc, n_cand, d_group, n_groups, d_pick, stream=None):
        """the buffer walk of the fast loop and PreModeDecision for n_groups blocks: d_group an array of md_fast_group_dtype(), d_pick
        one of md_fast_pick_dtype(); a group out of range is counted (inter_pred_refused)"""
        _check(lib().svthip_md_fast_pick_batch_dev(self._h, d_result, d_desc, n_cand, d_group, n_groups, d_pick, stream))
