"""CDEF (svthip_av1_[highbd_]cdef_search_mse_dev, svthip_cdef_pick_strengths_dev, .._cdef_search_dev, .._cdef_frame_dev,
svthip_cdef_dist_8x8_batch_dev): pointer marshalling only."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._core import _check, _hbd, _picture_ref, lib

CDEF_RESULT_DTYPE = np.dtype([("cdef_bits", "<i4"), ("nb_cdef_strengths", "<i4"), ("cdef_strengths", "<i4", (8,)), ("cdef_uv_strengths", "<i4", (8,)),
                              ("pri_damping", "<i4"), ("sec_damping", "<i4"), ("sb_count", "<i4")])
assert CDEF_RESULT_DTYPE.itemsize == 84
CDEF_PICK_MAX_FB = 4096


class CdefPicture(C.Structure):
    """svthip_cdef_picture: device pointers to sample (0, 0) of the deblocked, source and output planes, strides in samples, the luma size,
    the skip map (one byte per 4x4 luma cell) and its stride"""
    _fields_ = [("deblocked", C.c_void_p * 3), ("source", C.c_void_p * 3), ("out", C.c_void_p * 3), ("deblocked_stride", C.c_uint32 * 3),
                ("source_stride", C.c_uint32 * 3), ("out_stride", C.c_uint32 * 3), ("width", C.c_uint32), ("height", C.c_uint32),
                ("d_skip", C.c_void_p), ("skip_stride", C.c_uint32)]


def cdef_filter_blocks(width, height):
    """(nhfb, nvfb): 64x64 filter blocks each way"""
    return (width // 4 + 15) // 16, (height // 4 + 15) // 16


def make_cdef_picture(width, height, deblocked, deblocked_stride, d_skip, skip_stride, source=(None, None, None), source_stride=(0, 0, 0),
                      out=(None, None, None), out_stride=(0, 0, 0)):
    p = CdefPicture()
    for i in range(3):
        p.deblocked[i], p.source[i], p.out[i] = deblocked[i], source[i], out[i]
        p.deblocked_stride[i], p.source_stride[i], p.out_stride[i] = deblocked_stride[i], source_stride[i], out_stride[i]
    p.width, p.height, p.d_skip, p.skip_stride = width, height, d_skip, skip_stride
    return p


class Cdef:
    """the CDEF entries as Context methods; bit_depth selects the 8-bit or the highbd entry"""

    def av1_cdef_search_mse_dev(self, picture, base_qindex, d_mse, d_fb_counted, bit_depth=8, stream=None):
        f, bd = _hbd(bit_depth, "cdef_search_mse_dev")
        _check(f(self._h, _picture_ref(picture), base_qindex, *bd, d_mse, d_fb_counted, stream))

    def cdef_pick_strengths_dev(self, d_mse, d_fb_counted, nhfb, nvfb, base_qindex, bit_depth, d_result, d_fb_strength, stream=None):
        _check(lib().svthip_cdef_pick_strengths_dev(self._h, d_mse, d_fb_counted, nhfb, nvfb, base_qindex, bit_depth, d_result, d_fb_strength, stream))

    def av1_cdef_search_dev(self, picture, base_qindex, d_mse, d_fb_counted, d_result, d_fb_strength, bit_depth=8, stream=None):
        f, bd = _hbd(bit_depth, "cdef_search_dev")
        _check(f(self._h, _picture_ref(picture), base_qindex, *bd, d_mse, d_fb_counted, d_result, d_fb_strength, stream))

    def av1_cdef_frame_dev(self, picture, d_result, d_fb_strength, plane_start, plane_end, bit_depth=8, stream=None):
        f, bd = _hbd(bit_depth, "cdef_frame_dev")
        _check(f(self._h, _picture_ref(picture), d_result, d_fb_strength, plane_start, plane_end, *bd, stream))

    def cdef_dist_8x8_batch_dev(self, d_dst, d_src, n, coeff_shift, d_out, stream=None):
        _check(lib().svthip_cdef_dist_8x8_batch_dev(self._h, d_dst, d_src, n, coeff_shift, d_out, stream))
