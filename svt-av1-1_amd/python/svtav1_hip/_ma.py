"""Motion-analysis statistics behind ME and OIS: ZZ SADs, AC energy, distortion histograms, global motion, per-SB flags (include/svtav1_hip.h)."""
from __future__ import annotations

from . import _abi
from ._core import _check, lib
from ._me import PaPictureDesc

MaPictureParams = _abi.structure("svthip_ma_picture_params")
MA_PICTURE_PARAMS_DTYPE = _abi.dtype("svthip_ma_picture_params")


def make_ma_params(slice_is_intra=False, temporal_layer_index=0, hierarchical_levels=3, is_used_as_reference_flag=True, intensity_transition_flag=False,
                   ref_index=0):
    """One svthip_ma_picture_params"""
    p = MaPictureParams()
    p.slice_is_intra, p.temporal_layer_index, p.hierarchical_levels = int(slice_is_intra), int(temporal_layer_index), int(hierarchical_levels)
    p.is_used_as_reference_flag, p.intensity_transition_flag, p.ref_index = int(is_used_as_reference_flag), int(intensity_transition_flag), int(ref_index)
    return p


def _params(params):
    return (MaPictureParams * len(params))(*params)


class MotionAnalysis:
    """the motion-analysis entries as Context methods; every list argument has one entry per picture of the launch"""

    def ma_zz_sad_dev(self, d_pool, curs, prevs, d_sad, d_zz_cost, d_non_moving_index, stream=None):
        """ComputeDecimatedZzSad: the 1/16 planes of `curs` against the full-resolution planes of `prevs` (PaPictureDesc lists): d_sad [n][n_sb] u32,
        d_zz_cost, d_non_moving_index [n][n_sb] u8."""
        n = len(curs)
        assert len(prevs) == n, "one previous picture per current picture"
        _check(lib().svthip_ma_zz_sad_dev(self._h, d_pool, (PaPictureDesc * n)(*curs), (PaPictureDesc * n)(*prevs), n, d_sad, d_zz_cost, d_non_moving_index,
                                          stream))

    def ma_ac_energy_dev(self, d_pool, pics, params, d_y_mean, d_energy, d_mean, stream=None):
        """CalculateAcEnergy: d_energy, d_mean [n][n_sb][5] u64; the sentinel 100000000 outside complete SBs of intra pictures."""
        n = len(pics)
        assert len(params) == n, "one svthip_ma_picture_params per picture"
        _check(lib().svthip_ma_ac_energy_dev(self._h, d_pool, (PaPictureDesc * n)(*pics), _params(params), n, d_y_mean, d_energy, d_mean, stream))

    def ma_distortion_stats_dev(self, d_me, me_pu_stride, d_ois_cand, width, height, params, d_rc_me_distortion, d_inter_index, d_intra_index, d_histograms,
                                d_full_sb_count, stream=None):
        """rc_me_distortion and the distortion histograms: d_rc_me_distortion, d_inter_index, d_intra_index [n][n_sb] u32, d_histograms [n][2][128] u32
        (ME, OIS), d_full_sb_count [n] u32."""
        _check(lib().svthip_ma_distortion_stats_dev(self._h, d_me, me_pu_stride, d_ois_cand, width, height, _params(params), len(params), d_rc_me_distortion,
                                                    d_inter_index, d_intra_index, d_histograms, d_full_sb_count, stream))

    def ma_global_motion_dev(self, d_me, me_pu_stride, width, height, params, d_global_motion, stream=None):
        """MeBasedGlobalMotionDetection: d_global_motion [n][12] i32 = is_pan, is_tilt, panMvx, panMvy, tiltMvx, tiltMvy, five counters, rows without a
        list-0 candidate."""
        _check(lib().svthip_ma_global_motion_dev(self._h, d_me, me_pu_stride, width, height, _params(params), len(params), d_global_motion, stream))

    def ma_sb_flags_dev(self, d_y_mean, d_variance, d_ref_y_mean, d_ref_variance, ref_row_stride, n_ref_pics, d_me, me_pu_stride, d_ois_cand, width, height,
                        params, d_flags, stream=None):
        """DeriveSimilarCollocatedFlag, FailingMotionLcu, DetectUncoveredLcu: d_flags [n][n_sb][4] u8."""
        _check(lib().svthip_ma_sb_flags_dev(self._h, d_y_mean, d_variance, d_ref_y_mean, d_ref_variance, ref_row_stride, n_ref_pics, d_me, me_pu_stride,
                                            d_ois_cand, width, height, _params(params), len(params), d_flags, stream))
