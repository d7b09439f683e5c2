"""Mode decision's fast loop (svthip_md_fast_cost_batch_dev, svthip_md_fast_pick_batch_dev), its interpolation-filter search
(svthip_md_model_rd_batch_dev, svthip_md_interp_filter_search_batch_dev) and its full loop (svthip_md_full_loop_batch_dev, and svthip_md_full_loop128_batch_dev
for 128x128, 128x64 and 64x128), and its partition decision (svthip_md_partition_geometry, svthip_md_partition_batch_dev, _compose_dev, _picture_dev): pointer
marshalling only.

The four structs cross Python as numpy arrays in device memory; md_fast_desc_dtype() / md_fast_result_dtype() / md_fast_group_dtype() /
md_fast_pick_dtype() give their layouts (svthip_md_fast_desc, _result, _group, _pick of include/svtav1_hip.h); md_model_rd_desc_dtype() /
md_model_rd_result_dtype() / md_ifs_desc_dtype() / md_ifs_result_dtype() those of the search (svthip_md_model_rd_desc, _result,
svthip_md_ifs_desc, _result); md_full_desc_dtype() / md_full_result_dtype() / md_full_decision_dtype() / md_full128_tu_dtype() those of the full loop;
md_partition_block_dtype() / _sb_dtype() / _leaf_dtype() / _result_dtype() / _final_dtype() those of the partition decision."""
from __future__ import annotations

import numpy as np

from . import _abi
from ._core import _check, lib
from ._pred import _planes_arg

MD_FAST_LUMA_GIVEN, MD_FAST_SKIP_DISTORTION, MD_FAST_INVALID, MD_FAST_CHROMA_QUARTER, MD_FAST_TYPE_INTER, MD_FAST_MAX_CANDIDATES, MD_FAST_MAX_BUFFERS = (
    _abi.define("SVTHIP_MD_FAST_" + t) for t in ("LUMA_GIVEN", "SKIP_DISTORTION", "INVALID", "CHROMA_QUARTER", "TYPE_INTER", "MAX_CANDIDATES", "MAX_BUFFERS"))


def md_fast_desc_dtype() -> np.dtype:
    """svthip_md_fast_desc, 32 bytes; `lambda` is spelled lambda_"""
    return _abi.dtype("svthip_md_fast_desc", lambda_="lambda")


def md_fast_result_dtype() -> np.dtype:
    """svthip_md_fast_result, 16 bytes"""
    return _abi.dtype("svthip_md_fast_result")


def md_fast_group_dtype() -> np.dtype:
    """svthip_md_fast_group, 8 bytes"""
    return _abi.dtype("svthip_md_fast_group")


def md_fast_pick_dtype() -> np.dtype:
    """svthip_md_fast_pick, 32 bytes"""
    return _abi.dtype("svthip_md_fast_pick")


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


MD_IFS_SEARCH_FAST, MD_IFS_SEARCH_FULL = 1, 2
MD_IFS_REFUSED = 0xFF   # best_trial of a candidate refused on the device


def md_model_rd_desc_dtype() -> np.dtype:
    """svthip_md_model_rd_desc, 16 bytes; `lambda` is spelled lambda_"""
    return _abi.dtype("svthip_md_model_rd_desc", lambda_="lambda")


def md_model_rd_result_dtype() -> np.dtype:
    """svthip_md_model_rd_result, 32 bytes"""
    return _abi.dtype("svthip_md_model_rd_result")


def md_ifs_desc_dtype() -> np.dtype:
    """svthip_md_ifs_desc, 32 bytes; filter_rate[dir][filter], dir 0 the vertical (y) filter"""
    return _abi.dtype("svthip_md_ifs_desc", lambda_="lambda")


def md_ifs_result_dtype() -> np.dtype:
    """svthip_md_ifs_result, 32 bytes"""
    return _abi.dtype("svthip_md_ifs_result")


class InterpFilterSearch:
    """the interpolation-filter search entries as Context methods; planes are InterPlanes of 8-bit planes, the arrays device pointers"""

    def md_model_rd_batch_dev(self, src, pred, d_desc, n_tiles, bwidth, bheight, quantizer, d_result, stream=None):
        """SSE, modelled rate and distortion and RDCOST of n_tiles predicted tiles of one luma size (8x8 .. 128x128): d_desc an array of
        md_model_rd_desc_dtype(), d_result one of md_model_rd_result_dtype(); a tile at an odd position is counted (inter_pred_refused)"""
        _check(lib().svthip_md_model_rd_batch_dev(self._h, _planes_arg(src), _planes_arg(pred), d_desc, n_tiles, bwidth, bheight, quantizer, d_result,
                                                  stream))

    def md_interp_filter_search_batch_dev(self, ref0, ref1, src, d_pu_desc, d_ifs_desc, n_cand, bwidth, bheight, search_mode, enable_dual_filter,
                                          quantizer, write_back, d_result, stream=None):
        """interpolation_filter_search of n_cand candidates of one luma size: d_pu_desc a device array of INTER_PU_DESC_DTYPE (its
        interp_filters written when write_back), d_ifs_desc one of md_ifs_desc_dtype(), d_result one of md_ifs_result_dtype(); a refused
        candidate is counted (inter_pred_refused)"""
        _check(lib().svthip_md_interp_filter_search_batch_dev(self._h, _planes_arg(ref0), _planes_arg(ref1), _planes_arg(src), d_pu_desc, d_ifs_desc,
                                                              n_cand, bwidth, bheight, search_mode, enable_dual_filter, quantizer, write_back,
                                                              d_result, stream))


MD_FULL_LUMA, MD_FULL_CHROMA, MD_FULL_DECIDE, MD_FULL_MAX_SLOTS = (_abi.define("SVTHIP_MD_FULL_" + t) for t in ("LUMA", "CHROMA", "DECIDE", "MAX_SLOTS"))
MD_FULL_NONE = 0xFFFFFFFF   # row of an inactive slot, winner_row of a refused group


def md_full_desc_dtype() -> np.dtype:
    """svthip_md_full_desc, 48 bytes; `lambda` is spelled lambda_"""
    return _abi.dtype("svthip_md_full_desc", lambda_="lambda")


def md_full_result_dtype() -> np.dtype:
    """svthip_md_full_result, 144 bytes"""
    return _abi.dtype("svthip_md_full_result")


def md_full_decision_dtype() -> np.dtype:
    """svthip_md_full_decision, 16 bytes"""
    return _abi.dtype("svthip_md_full_decision")


def md_full_workspace_bytes(n_groups, max_full, bwidth, bheight, type_mask_inter, type_mask_intra) -> int:
    """bytes of d_work for a call of md_full_loop_batch_dev; 0 for arguments the entry refuses"""
    return int(lib().svthip_md_full_workspace_bytes(n_groups, max_full, bwidth, bheight, type_mask_inter, type_mask_intra))


def md_full128_tu_dtype() -> np.dtype:
    """svthip_md_full128_tu, 32 bytes: eob[plane][tu] of a slot of md_full_loop128_batch_dev"""
    return _abi.dtype("svthip_md_full128_tu")


def md_full128_workspace_bytes(n_groups, max_full, bwidth, bheight) -> int:
    """bytes of d_work for a call of md_full_loop128_batch_dev; 0 for arguments the entry refuses"""
    return int(lib().svthip_md_full128_workspace_bytes(n_groups, max_full, bwidth, bheight))


class ModeDecisionFull:
    """the full-loop entries as Context methods; planes are InterPlanes of 8-bit planes, the arrays device pointers"""

    def md_full_loop_batch_dev(self, src, pred, d_fast, d_full, n_cand, d_group, d_pick, n_groups, bwidth, bheight, d_qparams, d_iscan, iscan_offsets,
                               d_tables, reduced_tx_set, type_mask_inter, type_mask_intra, max_full, slot_recon, tiles_per_row, recon, d_work, stages,
                               d_result, d_decision, stream=None):
        """T/Q, rate, full cost, decision and the winner's reconstruction for n_groups blocks of one luma size: d_fast / d_group / d_pick the
        arrays of the fast loop, d_full one of md_full_desc_dtype(), iscan_offsets [19][16] host integers, d_work md_full_workspace_bytes(..)
        bytes, d_result n_groups * max_full rows of md_full_result_dtype(), d_decision n_groups of md_full_decision_dtype(); a group the pick
        refused or a TxType without a network is counted (inter_pred_refused)"""
        offsets = None if iscan_offsets is None else np.ascontiguousarray(np.asarray(iscan_offsets, np.uint32).reshape(19 * 16))
        _check(lib().svthip_md_full_loop_batch_dev(self._h, _planes_arg(src), _planes_arg(pred), d_fast, d_full, n_cand, d_group, d_pick, n_groups, bwidth,
                                                   bheight, d_qparams, d_iscan, None if offsets is None else offsets.ctypes.data, d_tables, reduced_tx_set,
                                                   type_mask_inter, type_mask_intra, max_full, _planes_arg(slot_recon), tiles_per_row, _planes_arg(recon),
                                                   d_work, stages, d_result, d_decision, stream))

    def md_full_loop128_batch_dev(self, src, pred, d_fast, d_full, n_cand, d_group, d_pick, n_groups, bwidth, bheight, d_qparams, d_iscan, iscan_offsets,
                                  d_tables, reduced_tx_set, max_full, slot_recon, tiles_per_row, recon, d_work, stages, d_result, d_tu, d_decision,
                                  stream=None):
        """md_full_loop_batch_dev for n_groups blocks of 128x128, 128x64 or 64x128 (2 or 4 luma TUs of 64x64 a block, no tx-type search):
        d_work md_full128_workspace_bytes(..) bytes, d_tu n_groups * max_full rows of md_full128_tu_dtype(); in d_result the has_coeff fields
        are bit masks over the TUs, quantized_dc the last TU's, eob TU 0's"""
        offsets = None if iscan_offsets is None else np.ascontiguousarray(np.asarray(iscan_offsets, np.uint32).reshape(19 * 16))
        _check(lib().svthip_md_full_loop128_batch_dev(self._h, _planes_arg(src), _planes_arg(pred), d_fast, d_full, n_cand, d_group, d_pick, n_groups,
                                                      bwidth, bheight, d_qparams, d_iscan, None if offsets is None else offsets.ctypes.data, d_tables,
                                                      reduced_tx_set, max_full, _planes_arg(slot_recon), tiles_per_row, _planes_arg(recon), d_work, stages,
                                                      d_result, d_tu, d_decision, stream))


MD_PART_NONE, MD_PART_SPLIT_FLAG, MD_PART_TESTED, MD_PART_MDC_SPLIT_FLAG, MD_PART_BLOCKS_64, MD_PART_BLOCKS_128, MD_PART_MAX_FINAL_64, MD_PART_MAX_FINAL_128 = (
    _abi.define("SVTHIP_MD_PART_" + t) for t in ("NONE", "SPLIT_FLAG", "TESTED", "MDC_SPLIT_FLAG", "BLOCKS_64", "BLOCKS_128", "MAX_FINAL_64", "MAX_FINAL_128"))


def md_partition_block_dtype() -> np.dtype:
    """svthip_md_partition_block, 16 bytes: a block of the md scan"""
    return _abi.dtype("svthip_md_partition_block")


def md_partition_sb_dtype() -> np.dtype:
    """svthip_md_partition_sb, 16 bytes"""
    return _abi.dtype("svthip_md_partition_sb")


def md_partition_leaf_dtype() -> np.dtype:
    """svthip_md_partition_leaf, 16 bytes"""
    return _abi.dtype("svthip_md_partition_leaf")


def md_partition_result_dtype() -> np.dtype:
    """svthip_md_partition_result, 16 bytes"""
    return _abi.dtype("svthip_md_partition_result")


def md_partition_final_dtype() -> np.dtype:
    """svthip_md_partition_final, 16 bytes"""
    return _abi.dtype("svthip_md_partition_final")


def md_partition_geometry(sb_size) -> np.ndarray:
    """the blocks of a 64x64 (1101) or 128x128 (4421) superblock in md-scan order, an array of md_partition_block_dtype(); host work, no context"""
    n = int(lib().svthip_md_partition_geometry(sb_size, None, 0))
    if not n:
        raise ValueError(f"sb_size must be 64 or 128, not {sb_size}")
    out = np.zeros(n, md_partition_block_dtype())
    assert int(lib().svthip_md_partition_geometry(sb_size, out.ctypes.data, n)) == n
    return out


def _fac_bits(partition_fac_bits):
    return None if partition_fac_bits is None else np.ascontiguousarray(np.asarray(partition_fac_bits, np.int32).reshape(20 * 11))


class ModeDecisionPartition:
    """the partition entries as Context methods; pool / dst are InterPlanes of 8-bit planes, the arrays device pointers"""

    def md_partition_batch_dev(self, d_sb, n_sb, d_leaf, n_leaf, d_decision, n_decision, sb_size, slice_is_intra, partition_fac_bits, d_result, d_final,
                               d_final_count, stream=None):
        """d1 and d2 over the block costs of n_sb superblocks and their final blocks in coding order: d_sb an array of md_partition_sb_dtype(),
        d_leaf one of md_partition_leaf_dtype(), d_decision the md_full_decision_dtype() rows the full-loop calls wrote, partition_fac_bits
        [20][11] host integers, d_result n_sb * MD_PART_BLOCKS_* rows of md_partition_result_dtype(), d_final n_sb * MD_PART_MAX_FINAL_* of
        md_partition_final_dtype(), d_final_count n_sb uint32; a bad leaf list and a final block without a leaf are counted (inter_pred_refused)"""
        bits = _fac_bits(partition_fac_bits)
        _check(lib().svthip_md_partition_batch_dev(self._h, d_sb, n_sb, d_leaf, n_leaf, d_decision, n_decision, sb_size, slice_is_intra,
                                                   None if bits is None else bits.ctypes.data, d_result, d_final, d_final_count, stream))

    def md_partition_compose_dev(self, n_sb, d_leaf, n_leaf, sb_size, d_final, d_final_count, pool, pool_width, pool_height, dst, width, height, stream=None):
        """the winner tiles of the final blocks, from `pool` at their leaves' pool_x / pool_y to `dst` at their picture positions; a block
        whose tile would pass a plane is skipped and counted (inter_pred_refused)"""
        _check(lib().svthip_md_partition_compose_dev(self._h, n_sb, d_leaf, n_leaf, sb_size, d_final, d_final_count, _planes_arg(pool), pool_width,
                                                     pool_height, _planes_arg(dst), width, height, stream))

    def md_partition_picture_dev(self, d_sb, n_sb, d_leaf, n_leaf, d_decision, n_decision, sb_size, slice_is_intra, partition_fac_bits, d_result, d_final,
                                 d_final_count, pool, pool_width, pool_height, dst, width, height, stream=None):
        """md_partition_batch_dev, then md_partition_compose_dev, on one stream"""
        bits = _fac_bits(partition_fac_bits)
        _check(lib().svthip_md_partition_picture_dev(self._h, d_sb, n_sb, d_leaf, n_leaf, d_decision, n_decision, sb_size, slice_is_intra,
                                                     None if bits is None else bits.ctypes.data, d_result, d_final, d_final_count, _planes_arg(pool),
                                                     pool_width, pool_height, _planes_arg(dst), width, height, stream))
