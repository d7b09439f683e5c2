"""Picture-analysis producers of the ME inputs and the open-loop intra search (include/svtav1_hip.h)."""
from __future__ import annotations

import ctypes as C

from ._core import _check, lib
from ._me import PaPictureDesc


class OisParams(C.Structure):
    _fields_ = [("slice_is_intra", C.c_uint8), ("temporal_layer_index", C.c_uint8), ("is_used_as_reference_flag", C.c_uint8),
                ("input_resolution_4k", C.c_uint8), ("limit_ois_to_dc_mode_flag", C.c_uint8), ("cu8x8_mode", C.c_uint8),
                ("enc_mode", C.c_uint8), ("reserved", C.c_uint8)]


class PictureAnalysis:
    """the picture-analysis and open-loop intra entries as Context methods"""

    def pa_derive_planes_dev(self, d_pool, pics, want_quarter=True, want_sixteenth=True, stream=None):
        """Pad the full-resolution planes and build the 1/4 and 1/16 planes of `pics` (PaPictureDesc list) inside the device pool."""
        n = len(pics)
        _check(lib().svthip_pa_derive_planes_dev(self._h, d_pool, (PaPictureDesc * n)(*pics), n, int(want_quarter), int(want_sixteenth), stream))

    def pad_plane_dev(self, d_plane, stride, width, height, pad_w, pad_h, sample_bytes=1, stream=None):
        """generate_padding / generate_padding16_bit of one device plane in place (all quantities in samples)."""
        _check(lib().svthip_pad_plane_dev(self._h, d_plane, stride, width, height, pad_w, pad_h, sample_bytes, stream))

    def open_loop_intra_search_batch_dev(self, d_pool, curs, params, d_sb, n_sb, d_me, me_pu_stride, d_cand, d_total, stream=None):
        """OpenLoopIntraSearchLcu over len(curs) pictures: d_cand [n][n_sb][85][18] u32 OisCandidate_t words, d_total [n][n_sb][85] u8."""
        n = len(curs)
        _check(lib().svthip_open_loop_intra_search_batch_dev(self._h, d_pool, (PaPictureDesc * n)(*curs), n, C.byref(params), d_sb, n_sb,
                                                             d_me, me_pu_stride, d_cand, d_total, stream))
