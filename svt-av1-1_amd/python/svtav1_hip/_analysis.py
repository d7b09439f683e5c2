"""Picture-analysis producers of the ME inputs and the open-loop intra search (include/svtav1_hip.h)."""
from __future__ import annotations

import ctypes as C

from . import _abi
from ._core import _check, lib
from ._me import PaPictureDesc

OisParams = _abi.structure("svthip_ois_params")


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


    def pa_unpack_10bit_dev(self, d_in16, in16, d_out8, out8, d_outn, outn, width, height, stream=None):
        """EB_ENC_msbUnPack2D over Y, Cb, Cr of len(in16) pictures: out8 = in >> 2, outn = in << 6 (bytes).  d_outn None: the 8-bit planes alone
        (UnPack8BitData).  in16 / out8 / outn: lists of make_planes(...), offsets and strides in samples from the base pointers."""
        n = len(in16)
        _check(lib().svthip_pa_unpack_10bit_dev(self._h, d_in16, _planes(in16, n), d_out8, _planes(out8, n), d_outn,
                                                _planes(outn, n) if d_outn else None, width, height, n, stream))

    def pa_pack_10bit_dev(self, d_in8, in8, d_inn, inn, d_out16, out16, width, height, compressed=False, stream=None):
        """EB_ENC_msbPack2D (compressed=False: inn unpacked 2-bit planes) or CompressedPackmsb (compressed=True: inn the SB-tiled compressed
        planes, offsets in bytes, strides not read) over Y, Cb, Cr of len(in8) pictures: out16 = (in8 << 2) | 2-bit."""
        n = len(in8)
        fn = lib().svthip_pa_pack_10bit_compressed_dev if compressed else lib().svthip_pa_pack_10bit_dev
        _check(fn(self._h, d_in8, _planes(in8, n), d_inn, _planes(inn, n), d_out16, _planes(out16, n), width, height, n, stream))

    def picture_sse_dev(self, d_recon, recon, d_src, src, width, height, d_sse, stream=None):
        """PsnrCalculations at 8 bits: d_sse [len(recon)][3] u64, the sums of squared differences of Y, Cb, Cr."""
        n = len(recon)
        _check(lib().svthip_picture_sse_dev(self._h, d_recon, _planes(recon, n), d_src, _planes(src, n), width, height, n, d_sse, stream))

    def highbd_picture_sse_dev(self, d_recon, recon, source_form, d_src, src, d_srcn, srcn, width, height, d_sse, stream=None):
        """PsnrCalculations at 16 bits against a source in form SSE_SRC_16BIT (d_src 16-bit planes), SSE_SRC_UNPACKED (d_src 8-bit, d_srcn
        unpacked 2-bit planes) or SSE_SRC_COMPRESSED (d_srcn the compressed planes): d_sse [len(recon)][3] u64."""
        n = len(recon)
        _check(lib().svthip_highbd_picture_sse_dev(self._h, d_recon, _planes(recon, n), source_form, d_src, _planes(src, n), d_srcn,
                                                   _planes(srcn, n) if srcn is not None else None, width, height, n, d_sse, stream))


SSE_SRC_16BIT = _abi.define("SVTHIP_SSE_SRC_16BIT")
SSE_SRC_UNPACKED = _abi.define("SVTHIP_SSE_SRC_UNPACKED")
SSE_SRC_COMPRESSED = _abi.define("SVTHIP_SSE_SRC_COMPRESSED")
_Planes = _abi.structure("svthip_planes")


def make_planes(offsets, strides):
    """One svthip_planes: the offsets of sample (0, 0) of Y, Cb, Cr from a base pointer and the strides, in samples."""
    p = _Planes()
    p.offset[:], p.stride[:] = [int(v) for v in offsets], [int(v) for v in strides]
    return p


def _planes(planes, n):
    assert len(planes) == n, "one svthip_planes per picture in every set"
    return (_Planes * n)(*planes)


def _chroma_offsets(chroma_offsets, n):
    """[n][2] pool offsets as the int64_t array the entries take"""
    flat = [int(v) for pair in chroma_offsets for v in pair]
    assert len(flat) == 2 * n, "one (Cb, Cr) offset pair per picture"
    return (C.c_int64 * (2 * n))(*flat)
