"""The deblocking filter and its level search (svthip_av1_[highbd_]loop_filter_frame_dev, .._loop_filter_sse_table_dev,
svthip_lf_level_walk_dev, svthip_av1_[highbd_]pick_filter_level_dev)."""
from __future__ import annotations

import ctypes as C

from . import _abi
from ._core import _check, _picture_ref, lib

LF_MI_DTYPE = _abi.dtype("svthip_lf_mi")
# svthip_lf_picture: device pointers to sample (0, 0) of the planes, strides in samples, the luma size
LfPicture = _abi.structure("svthip_lf_picture")


def make_lf_picture(width, height, recon, recon_stride, source=(None, None, None), source_stride=(0, 0, 0)):
    p = LfPicture()
    for i in range(3):
        p.recon[i], p.source[i], p.recon_stride[i], p.source_stride[i] = recon[i], source[i], recon_stride[i], source_stride[i]
    p.width, p.height = width, height
    return p


class Deblocking:
    """the deblocking entries as Context methods; bit_depth selects the 8-bit or the highbd entry"""

    def av1_loop_filter_frame_dev(self, picture, d_mi, mi_stride, d_levels, sharpness, plane_start, plane_end, bit_depth=8, stream=None):
        """av1_loop_filter_frame on planes [plane_start, plane_end) in place; d_mi a device grid of LF_MI_DTYPE, d_levels four int32 on the device."""
        if bit_depth == 8:
            _check(lib().svthip_av1_loop_filter_frame_dev(self._h, _picture_ref(picture), d_mi, mi_stride, d_levels, sharpness, plane_start, plane_end, stream))
        else:
            _check(lib().svthip_av1_highbd_loop_filter_frame_dev(self._h, _picture_ref(picture), d_mi, mi_stride, d_levels, sharpness, plane_start,
                                                                 plane_end, bit_depth, stream))

    def av1_loop_filter_sse_table_dev(self, picture, d_mi, mi_stride, plane, direction, d_levels, sharpness, d_sse, bit_depth=8, stream=None):
        """d_sse[64] (uint64): try_filter_frame's result for every level of (plane, direction)."""
        if bit_depth == 8:
            _check(lib().svthip_av1_loop_filter_sse_table_dev(self._h, _picture_ref(picture), d_mi, mi_stride, plane, direction, d_levels, sharpness, d_sse,
                                                              stream))
        else:
            _check(lib().svthip_av1_highbd_loop_filter_sse_table_dev(self._h, _picture_ref(picture), d_mi, mi_stride, plane, direction, d_levels, sharpness,
                                                                     bit_depth, d_sse, stream))

    def lf_level_walk_dev(self, d_sse, start_level, only_4x4, d_level_out, d_visited=None, stream=None):
        """search_filter_level's walk over a table of 64 sums: the level (int32) and the mask of the levels it asked for (uint64)."""
        _check(lib().svthip_lf_level_walk_dev(self._h, d_sse, start_level, int(only_4x4), d_level_out, d_visited, stream))

    def av1_pick_filter_level_dev(self, picture, d_mi, mi_stride, last_levels, sharpness, only_4x4, d_levels, d_sse_tables, d_visited=None, bit_depth=8,
                                  stream=None):
        """av1_pick_filter_level(LPF_PICK_FROM_FULL_IMAGE): the four levels into d_levels, the five tables into d_sse_tables[5][64]."""
        last = (C.c_int32 * 4)(*[int(v) for v in last_levels]) if last_levels is not None else None
        if bit_depth == 8:
            _check(lib().svthip_av1_pick_filter_level_dev(self._h, _picture_ref(picture), d_mi, mi_stride, last, sharpness, int(only_4x4), d_levels,
                                                          d_sse_tables, d_visited, stream))
        else:
            _check(lib().svthip_av1_highbd_pick_filter_level_dev(self._h, _picture_ref(picture), d_mi, mi_stride, last, sharpness, int(only_4x4), bit_depth,
                                                                 d_levels, d_sse_tables, d_visited, stream))
