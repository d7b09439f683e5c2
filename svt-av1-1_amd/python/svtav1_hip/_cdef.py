"""CDEF (svthip_av1_[highbd_]cdef_search_mse_dev, svthip_cdef_pick_strengths_dev, .._cdef_search_dev, .._cdef_frame_dev,
svthip_cdef_dist_8x8_batch_dev, and the ..128 entries for grids with 128-wide blocks): pointer marshalling only."""
from __future__ import annotations

from . import _abi
from ._core import _check, _hbd, _picture_ref, lib

CDEF_RESULT_DTYPE = _abi.dtype("svthip_cdef_result")
CDEF_PICK_MAX_FB = _abi.define("SVTHIP_CDEF_PICK_MAX_FB")
# svthip_cdef_picture: device pointers to sample (0, 0) of the deblocked, source and output planes, strides in samples, the luma size,
# the skip map (one byte per 4x4 luma cell) and its stride
CdefPicture = _abi.structure("svthip_cdef_picture")


def cdef_filter_blocks(width, height):
    """(nhfb, nvfb): 64x64 filter blocks each way"""
    return (width // 4 + 15) // 16, (height // 4 + 15) // 16


def cdef_search128_workspace_bytes(width, height) -> int:
    """bytes of d_workspace for the ..search[_mse]128_dev entries; 0 for a size the entries refuse"""
    return int(lib().svthip_cdef_search128_workspace_bytes(width, height))


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

    def av1_cdef_search_mse128_dev(self, picture, base_qindex, d_mse, d_fb_counted, d_mi, mi_stride, d_workspace, bit_depth=8, stream=None):
        """d_mi: the svthip_lf_mi grid of the deblocking entries (sb_type of each fb's first cell is read)"""
        f, bd = _hbd(bit_depth, "cdef_search_mse128_dev")
        _check(f(self._h, _picture_ref(picture), base_qindex, *bd, d_mse, d_fb_counted, d_mi, mi_stride, d_workspace, stream))

    def cdef_pick_strengths128_dev(self, d_mse, d_fb_counted, nhfb, nvfb, base_qindex, bit_depth, d_result, d_fb_strength, d_mi, mi_stride, stream=None):
        _check(lib().svthip_cdef_pick_strengths128_dev(self._h, d_mse, d_fb_counted, nhfb, nvfb, base_qindex, bit_depth, d_result, d_fb_strength, d_mi,
                                                       mi_stride, stream))

    def av1_cdef_search128_dev(self, picture, base_qindex, d_mse, d_fb_counted, d_result, d_fb_strength, d_mi, mi_stride, d_workspace, bit_depth=8,
                               stream=None):
        f, bd = _hbd(bit_depth, "cdef_search128_dev")
        _check(f(self._h, _picture_ref(picture), base_qindex, *bd, d_mse, d_fb_counted, d_result, d_fb_strength, d_mi, mi_stride, d_workspace, stream))

    def av1_cdef_frame_dev(self, picture, d_result, d_fb_strength, plane_start, plane_end, bit_depth=8, stream=None):
        f, bd = _hbd(bit_depth, "cdef_frame_dev")
        _check(f(self._h, _picture_ref(picture), d_result, d_fb_strength, plane_start, plane_end, *bd, stream))

    def cdef_dist_8x8_batch_dev(self, d_dst, d_src, n, coeff_shift, d_out, stream=None):
        _check(lib().svthip_cdef_dist_8x8_batch_dev(self._h, d_dst, d_src, n, coeff_shift, d_out, stream))
