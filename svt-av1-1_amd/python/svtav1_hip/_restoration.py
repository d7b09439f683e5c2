"""Loop restoration, pointer marshalling only.  Wiener: svthip_av1_[highbd_]wiener_stats_dev, svthip_wiener_solve_dev, .._wiener_trial_sse_dev,
svthip_wiener_walk_init_dev / _step_dev, .._search_wiener_dev, .._loop_restoration_filter_frame_dev.  Self-guided:
svthip_av1_[highbd_]selfguided_restoration_dev, svthip_sgrproj_solve_dev, svthip_sgrproj_walk_table_dev, .._search_sgrproj_dev,
.._sgrproj_trial_sse_dev, .._lr_filter_frame_dev.  The decision: svthip_rest_finish_search_dev, and the whole stage in one call:
svthip_av1_[highbd_]pick_filter_restoration_dev."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._core import _check, _hbd, _picture_ref, lib

RESTORE_NONE, RESTORE_WIENER, RESTORE_SGRPROJ, RESTORE_SWITCHABLE = (_abi.define("SVTHIP_RESTORE_" + t) for t in ("NONE", "WIENER", "SGRPROJ", "SWITCHABLE"))
WIENER_WALK_STATE_DTYPE = _abi.dtype("svthip_wiener_walk_state")

SGRPROJ_DETAIL_DTYPE = _abi.dtype("svthip_sgrproj_detail")
SGRPROJ_PARAMS = 16
# svthip_lr_picture: device pointers to sample (0, 0) of the CDEF'd, deblocked and source planes, strides in samples, the luma size, the
# restoration unit size per plane
LrPicture = _abi.structure("svthip_lr_picture")


def lr_unit_sizes(width, height):
    """the reference's choice (EbPictureControlSet.c:32-47)"""
    luma = 256 if width * height > 352 * 288 else 128
    return (luma, luma // 2, luma // 2)


def make_lr_picture(width, height, cdef, cdef_stride, deblocked, deblocked_stride, source=(None, None, None), source_stride=(0, 0, 0), unit_size=None):
    p = LrPicture()
    unit_size = unit_size or lr_unit_sizes(width, height)
    for i in range(3):
        p.cdef[i], p.deblocked[i], p.source[i] = cdef[i], deblocked[i], source[i]
        p.cdef_stride[i], p.deblocked_stride[i], p.source_stride[i], p.unit_size[i] = cdef_stride[i], deblocked_stride[i], source_stride[i], unit_size[i]
    p.width, p.height = width, height
    return p


def lr_unit_geometry(width, height, unit_size=None):
    """(unit_base[4], limits[units][4] = h_start, h_end, v_start, v_end) from the library's own geometry (the one the kernels launch with)"""
    us = (C.c_uint32 * 3)(*(unit_size or lr_unit_sizes(width, height)))
    base = (C.c_uint32 * 4)()
    n = lib().svthip_lr_unit_geometry(width, height, us, base, None)
    limits = np.zeros((n, 4), np.int32)
    lib().svthip_lr_unit_geometry(width, height, us, base, limits.ctypes.data)
    return [int(b) for b in base], limits


def lr_workspace_bytes(n_units):
    return int(lib().svthip_lr_workspace_bytes(n_units))


def wiener_walk_max_trials(wiener_win=7):
    return int(lib().svthip_wiener_walk_max_trials(wiener_win))


def sgrproj_workspace_bytes(width, height):
    return int(lib().svthip_sgrproj_workspace_bytes(width, height))


def sgrproj_walk_max_trials():
    return int(lib().svthip_sgrproj_walk_max_trials())


def lr_pick_workspace_bytes(width, height, unit_size=None):
    """bytes of d_work for av1_pick_filter_restoration_dev; 0 for a size the entries refuse"""
    return int(lib().svthip_lr_pick_workspace_bytes(width, height, (C.c_uint32 * 3)(*(unit_size or lr_unit_sizes(width, height)))))


def rest_finish_rates_dtype() -> np.dtype:
    """svthip_rest_finish_rates, 32 bytes, host memory"""
    return _abi.dtype("svthip_rest_finish_rates")


def rest_finish_result_dtype() -> np.dtype:
    """svthip_rest_finish_result, 104 bytes, one per plane; sse, bits and cost are indexed by frame type"""
    return _abi.dtype("svthip_rest_finish_result")


def _rates_ref(rates):
    """a pointer to one svthip_rest_finish_rates from a record of rest_finish_rates_dtype(), a mapping or (rdmult, wiener, sgrproj, switchable);
    the second value keeps the memory alive for the call"""
    if rates is None:
        return None, None
    if isinstance(rates, dict):
        rates = (rates["rdmult"], rates["wiener_cost"], rates["sgrproj_cost"], rates["switchable_cost"])
    a = np.zeros(1, rest_finish_rates_dtype())
    a[0] = tuple(rates) if not isinstance(rates, np.void) else rates
    return a.ctypes.data, a


class Restoration:
    """the loop-restoration entries as Context methods; bit_depth selects the 8-bit or the highbd entry"""

    def av1_wiener_stats_dev(self, picture, plane_start, plane_end, d_M, d_H, d_avg, d_sse_none, d_work, bit_depth=8, stream=None):
        f, bd = _hbd(bit_depth, "wiener_stats_dev")
        _check(f(self._h, _picture_ref(picture), plane_start, plane_end, *bd, d_M, d_H, d_avg, d_sse_none, d_work, stream))

    def wiener_solve_dev(self, d_M, d_H, unit_begin, unit_end, wiener_win, d_taps, d_rejected, stream=None):
        _check(lib().svthip_wiener_solve_dev(self._h, d_M, d_H, unit_begin, unit_end, wiener_win, d_taps, d_rejected, stream))

    def av1_wiener_trial_sse_dev(self, picture, plane_start, plane_end, d_taps, d_sse, d_skip=None, bit_depth=8, stream=None):
        f, bd = _hbd(bit_depth, "wiener_trial_sse_dev")
        _check(f(self._h, _picture_ref(picture), plane_start, plane_end, *bd, d_taps, d_skip, d_sse, stream))

    def wiener_walk_init_dev(self, d_state, d_taps, d_rejected, unit_begin, unit_end, wiener_win, stream=None):
        _check(lib().svthip_wiener_walk_init_dev(self._h, d_state, d_taps, d_rejected, unit_begin, unit_end, wiener_win, stream))

    def wiener_walk_step_dev(self, d_state, d_trial_sse, unit_begin, unit_end, d_pending=None, stream=None):
        _check(lib().svthip_wiener_walk_step_dev(self._h, d_state, d_trial_sse, unit_begin, unit_end, d_pending, stream))

    def av1_search_wiener_dev(self, picture, plane_start, plane_end, d_work, d_sse, d_taps, d_n_trials, d_pending, n_steps=0, resume=False, bit_depth=8,
                              stream=None):
        f, bd = _hbd(bit_depth, "search_wiener_dev")
        _check(f(self._h, _picture_ref(picture), plane_start, plane_end, *bd, n_steps, int(resume), d_work, d_sse, d_taps, d_n_trials, d_pending, stream))

    def av1_loop_restoration_filter_frame_dev(self, picture, d_out, out_stride, plane_start, plane_end, d_unit_type, d_taps, bit_depth=8, stream=None):
        f, bd = _hbd(bit_depth, "loop_restoration_filter_frame_dev")
        out = (C.c_void_p * 3)(*d_out) if d_out is not None else None
        strides = (C.c_uint32 * 3)(*out_stride) if out_stride is not None else None
        _check(f(self._h, _picture_ref(picture), out, strides, plane_start, plane_end, *bd, d_unit_type, d_taps, stream))

    def av1_selfguided_restoration_dev(self, picture, plane, ep, d_flt0, d_flt1, flt_stride, bit_depth=8, stream=None):
        f, bd = _hbd(bit_depth, "selfguided_restoration_dev")
        _check(f(self._h, _picture_ref(picture), plane, *bd, ep, d_flt0, d_flt1, flt_stride, stream))

    def sgrproj_solve_dev(self, d_sums, d_size, d_ep, n, d_xq, d_xqd, stream=None):
        _check(lib().svthip_sgrproj_solve_dev(self._h, d_sums, d_size, d_ep, n, d_xq, d_xqd, stream))

    def sgrproj_walk_table_dev(self, d_err, d_ep, d_start_xqd, n, d_xqd, d_best_err, d_n_trials, stream=None):
        _check(lib().svthip_sgrproj_walk_table_dev(self._h, d_err, d_ep, d_start_xqd, n, d_xqd, d_best_err, d_n_trials, stream))

    def av1_search_sgrproj_dev(self, picture, plane_start, plane_end, d_work, d_sgrproj, d_sse, d_detail=None, bit_depth=8, stream=None):
        f, bd = _hbd(bit_depth, "search_sgrproj_dev")
        _check(f(self._h, _picture_ref(picture), plane_start, plane_end, *bd, d_work, d_sgrproj, d_sse, d_detail, stream))

    def av1_sgrproj_trial_sse_dev(self, picture, plane_start, plane_end, d_sgrproj, d_sse, d_skip=None, bit_depth=8, stream=None):
        f, bd = _hbd(bit_depth, "sgrproj_trial_sse_dev")
        _check(f(self._h, _picture_ref(picture), plane_start, plane_end, *bd, d_sgrproj, d_skip, d_sse, stream))

    def av1_lr_filter_frame_dev(self, picture, d_out, out_stride, plane_start, plane_end, d_unit_type, d_taps, d_sgrproj, bit_depth=8, stream=None):
        f, bd = _hbd(bit_depth, "lr_filter_frame_dev")
        out = (C.c_void_p * 3)(*d_out) if d_out is not None else None
        strides = (C.c_uint32 * 3)(*out_stride) if out_stride is not None else None
        _check(f(self._h, _picture_ref(picture), out, strides, plane_start, plane_end, *bd, d_unit_type, d_taps, d_sgrproj, stream))

    def rest_finish_search_dev(self, rates, unit_base, plane_start, plane_end, d_wiener_sse, d_taps, d_sgr_sse, d_sgrproj, d_unit_type, d_result,
                               d_best_rtype=None, stream=None):
        """rest_finish_search on the searches' tables: unit types, frame types and results of planes [plane_start, plane_end)"""
        r, keep = _rates_ref(rates)
        base = (C.c_uint32 * 4)(*unit_base) if unit_base is not None else None
        _check(lib().svthip_rest_finish_search_dev(self._h, r, base, plane_start, plane_end, d_wiener_sse, d_taps, d_sgr_sse, d_sgrproj, d_unit_type,
                                                   d_best_rtype, d_result, stream))
        del keep

    def av1_pick_filter_restoration_dev(self, picture, rates, d_work, d_out, out_stride, d_unit_type, d_taps, d_sgrproj, d_result, bit_depth=8, stream=None):
        """both searches, the decision and the frame filter of the three planes in one call"""
        f, bd = _hbd(bit_depth, "pick_filter_restoration_dev")
        r, keep = _rates_ref(rates)
        out = (C.c_void_p * 3)(*d_out) if d_out is not None else None
        strides = (C.c_uint32 * 3)(*out_stride) if out_stride is not None else None
        _check(f(self._h, _picture_ref(picture), *bd, r, d_work, out, strides, d_unit_type, d_taps, d_sgrproj, d_result, stream))
        del keep
