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

    def pa_block_stats_dev(self, d_pool, pics, chroma_offsets, chroma_stride, sub_precision, d_y_mean, d_variance, d_cb_mean, d_cr_mean, stream=None):
        """ComputeBlockMeanComputeVariance / ComputeChromaBlockMean over len(pics) pictures of equal size: d_y_mean, d_variance [n][n_sb][85],
        d_cb_mean, d_cr_mean [n][n_sb][21].  chroma_offsets: per picture the pool offsets of Cb and Cr sample (0, 0)."""
        n = len(pics)
        _check(lib().svthip_pa_block_stats_dev(self._h, d_pool, (PaPictureDesc * n)(*pics), n, _chroma_offsets(chroma_offsets, n), chroma_stride,
                                               int(sub_precision), d_y_mean, d_variance, d_cb_mean, d_cr_mean, stream))

    def pa_homogeneity_dev(self, d_variance, width, height, n_pics, d_var_of_var32x32, d_homogeneous, d_picture, stream=None):
        """DetermineHomogeneousRegionInPicture and pic_avg_variance from d_variance: d_var_of_var32x32 [n][n_sb][4] u64, d_homogeneous
        [n][n_sb] u8, d_picture [n][4] u32 = pic_avg_variance, very_low_var_pic_flag, logo_pic_flag, complete SBs."""
        _check(lib().svthip_pa_homogeneity_dev(self._h, d_variance, width, height, n_pics, d_var_of_var32x32, d_homogeneous, d_picture, stream))

    def pa_histograms_dev(self, d_pool, pics, chroma_offsets, chroma_stride, d_histogram, d_region_intensity, d_average_intensity, stream=None):
        """The SCD_MODE_1 histograms and intensities: d_histogram [n][4][4][3][256] u32, d_region_intensity [n][4][4][3] u32,
        d_average_intensity [n][3] u32."""
        n = len(pics)
        _check(lib().svthip_pa_histograms_dev(self._h, d_pool, (PaPictureDesc * n)(*pics), n, _chroma_offsets(chroma_offsets, n), chroma_stride,
                                              d_histogram, d_region_intensity, d_average_intensity, stream))

    def pa_noise_detect_dev(self, d_pool, pics, sub_precision, d_denoised, denoised_stride, d_sb_var, d_flat_noise, d_picture, stream=None):
        """DetectInputPictureNoise over len(pics) pictures of equal size, before the borders exist: d_sb_var [n][n_sb][2] u64 (noise variance
        raw, denoised variance >> 16), d_flat_noise [n][n_sb] u8, d_picture [n][4] u32 = sum, complete SBs, pic_noise_class, sum >= count.
        d_denoised: None (detection only) or [n][height][denoised_stride] u8 for the denoised luma."""
        n = len(pics)
        _check(lib().svthip_pa_noise_detect_dev(self._h, d_pool, (PaPictureDesc * n)(*pics), n, int(sub_precision), d_denoised, denoised_stride,
                                                d_sb_var, d_flat_noise, d_picture, stream))

    def pa_denoise_dev(self, d_pool, pics, chroma_offsets, chroma_stride, d_denoised, denoised_stride, d_flat_noise, d_picture, stream=None):
        """DenoiseInputPicture in place on the pool, the arm chosen on the device from d_picture; d_denoised is used up as chroma scratch."""
        n = len(pics)
        _check(lib().svthip_pa_denoise_dev(self._h, d_pool, (PaPictureDesc * n)(*pics), n, _chroma_offsets(chroma_offsets, n), chroma_stride,
                                           d_denoised, denoised_stride, d_flat_noise, d_picture, stream))


def _chroma_offsets(chroma_offsets, n):
    """[n][2] pool offsets as the int64_t array the entries take"""
    flat = [int(v) for pair in chroma_offsets for v in pair]
    assert len(flat) == 2 * n, "one (Cb, Cr) offset pair per picture"
    return (C.c_int64 * (2 * n))(*flat)
