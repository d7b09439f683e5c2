"""Motion estimation (include/svtav1_hip.h: full-pel search, HME, sub-pel refinement, bi-prediction and packing, whole-picture ME,
SadLoopKernel): descriptors, parameter blocks and the Context methods."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._core import _check, lib

NUM_SQ_PU = _abi.define("SVTHIP_NUM_SQ_PU")
MAX_SAD_VALUE = _abi.define("SVTHIP_MAX_SAD_VALUE")
HME_MAX_JOBS = _abi.define("SVTHIP_HME_MAX_JOBS")  # pictures per kernel launch of the batch entries
# MeContext_t::fractionalSearchMethod
FRACTIONAL_SUB_SAD_SEARCH = _abi.define("SVTHIP_FRACTIONAL_SUB_SAD_SEARCH")
FRACTIONAL_FULL_SAD_SEARCH = _abi.define("SVTHIP_FRACTIONAL_FULL_SAD_SEARCH")
FRACTIONAL_SSD_SEARCH = _abi.define("SVTHIP_FRACTIONAL_SSD_SEARCH")

FullpelDesc = _abi.structure("svthip_fullpel_desc")
PaPictureDesc = _abi.structure("svthip_pa_picture")
MeParams = _abi.structure("svthip_me_params")
MeCuResult = _abi.structure("svthip_me_cu_result")
ME_CU_RESULT_DTYPE = _abi.dtype("svthip_me_cu_result")
assert ME_CU_RESULT_DTYPE.itemsize == C.sizeof(MeCuResult) == 24
SbOrigin = _abi.structure("svthip_sb_origin")
# in-loop motion estimation: 849 blocks per 64x64 superblock
INLOOP_ME_PU_COUNT = _abi.define("SVTHIP_INLOOP_ME_PU_COUNT")
INLOOP_BLOCKS_ALL = _abi.define("SVTHIP_INLOOP_BLOCKS_ALL")
INLOOP_BLOCKS_SIDE_4 = _abi.define("SVTHIP_INLOOP_BLOCKS_SIDE_4")
InloopDesc = _abi.structure("svthip_inloop_desc")
INLOOP_DESC_DTYPE = _abi.dtype("svthip_inloop_desc")

# HME_LEVEL_0_SEARCH_AREA_MULTIPLIER_X / _Y [hierarchical_levels][temporal_layer_index]
# (Codec/EbDefinitions.h:2980-2996); X and Y tables are identical in the reference.
HME_LEVEL0_MULTIPLIER = [[100], [100, 100], [100, 100, 100], [200, 140, 100, 70], [350, 200, 100, 100, 100],
                         [525, 350, 200, 100, 100, 100]]


def default_me_params(width: int, height: int, hierarchical_levels: int = 3, temporal_layer_index: int = 0,
                      is_ref: bool = True, ref_poc_equal: bool = False) -> MeParams:
    """set_me_hme_params_oq() for enc modes M0..M3 (column 0 of the tables, Codec/EbDefinitions.h:3332-3465;
    resolution class per Codec/EbMotionEstimationProcess.c:104-110)."""
    px = width * height
    ratio = width // height
    if px < 1280 * 720 * 0.75:  # INPUT_SIZE_576p_RANGE_OR_LOWER (Codec/EbDefinitions.h input-size thresholds)
        ri = 0
    elif px < 1920 * 1080 * 0.75 and ratio < 2:
        ri = 1
    elif px <= 1920 * 1088 * 1.5:
        ri = 3
    else:
        ri = 4
    tot_w = [48, 64, 96, 96, 128][ri]
    tot_h = [40, 48, 48, 48, 80][ri]
    p = MeParams()
    p.search_area_width, p.search_area_height = 64, 64
    p.number_hme_search_region_in_width = p.number_hme_search_region_in_height = 2
    p.hme_level0_total_search_area_width, p.hme_level0_total_search_area_height = tot_w, tot_h
    for k in range(2):
        p.hme_level0_search_area_in_width_array[k] = tot_w // 2
        p.hme_level0_search_area_in_height_array[k] = tot_h // 2
        p.hme_level1_search_area_in_width_array[k] = 16
        p.hme_level1_search_area_in_height_array[k] = 16
        p.hme_level2_search_area_in_width_array[k] = 8
        p.hme_level2_search_area_in_height_array[k] = 8
    m = HME_LEVEL0_MULTIPLIER[hierarchical_levels][temporal_layer_index]
    p.hme_level0_multiplier_x = p.hme_level0_multiplier_y = m
    p.enable_hme_flag = p.enable_hme_level0_flag = p.enable_hme_level1_flag = p.enable_hme_level2_flag = 1
    p.temporal_layer_index = temporal_layer_index
    p.is_used_as_reference_flag = int(is_ref)
    p.ref_poc_equal = int(ref_poc_equal)
    return p


def make_fullpel_desc(cur, ref, centers=None, search_w=64, search_h=64) -> np.ndarray:
    """Descriptors for every SB of a picture the way MotionEstimateLcu derives them
    (Codec/EbMotionEstimation.c:6667-6738): window centred on `centers[sb] = (x, y)` (default 0,0),
    clipped to the picture, source block at the SB origin."""
    from . import synth

    nx, ny = cur.sb_grid()
    out = np.zeros((nx * ny, 6), dtype=np.int32)
    for sy in range(ny):
        for sx in range(nx):
            i = sy * nx + sx
            ox, oy = sx * 64, sy * 64
            cx, cy = (0, 0) if centers is None else centers[i]
            xo, yo, sw, sh = synth.clamp_search_window(ox, oy, int(cx), int(cy), search_w, search_h, cur.width, cur.height)
            out[i] = [(synth.PAD_FULL + oy) * cur.stride + synth.PAD_FULL + ox,
                      (synth.PAD_FULL + oy + yo) * ref.stride + synth.PAD_FULL + ox + xo, xo, yo, sw, sh]
    return out


def build_picture_pool(pictures):
    """Stack the three planes of each PaPicture into one uint8 pool (4-byte aligned planes).
    Returns (pool, [PaPictureDesc])."""
    chunks, descs, off = [], [], 0
    for p in pictures:
        d = PaPictureDesc()
        for name, arr in (("full", p.full), ("quarter", p.quarter), ("sixteenth", p.sixteenth)):
            flat = arr.reshape(-1)
            padn = (-flat.size) % 16
            setattr(d, name + "_offset", off)
            setattr(d, name + "_stride", arr.shape[1])
            chunks.append(flat)
            if padn:
                chunks.append(np.zeros(padn, np.uint8))
            off += flat.size + padn
        d.width, d.height = p.width, p.height
        descs.append(d)
    chunks.append(np.zeros(256, np.uint8))   # the kernels' aligned-group loads may run up to 64 bytes past the last plane
    return np.concatenate(chunks), descs


def sb_origins(width: int, height: int) -> np.ndarray:
    nx, ny = (width + 63) // 64, (height + 63) // 64
    out = np.zeros((nx * ny, 2), dtype=np.uint16)
    for sy in range(ny):
        for sx in range(nx):
            out[sy * nx + sx] = (sx * 64, sy * 64)
    return out


def shard_sb_rows(width: int, height: int, world: int, rank: int) -> np.ndarray:
    """Contiguous SB-ROW partition of one picture across `world` ranks (1080p -> 17 rows -> 3/2/2/...): the indices
    (into sb_origins(width, height)) of the SBs rank `rank` owns.  See svtav1_hip.sharded for the multi-GPU layer built on it."""
    from .sharded import shard_sb_indices

    return shard_sb_indices(width, height, world, rank, "row")


class MotionEstimation:
    """the motion-estimation entries as Context methods"""

    # -- host-pointer form (numpy in / numpy out) ------------------------------------------------
    def fullpel_search(self, src_plane: np.ndarray, ref_plane: np.ndarray, desc: np.ndarray):
        """desc int32 [n,6] -> (best_sad [n,85] uint32, best_mv [n,85] uint32)."""
        assert src_plane.dtype == np.uint8 and ref_plane.dtype == np.uint8
        src_plane = np.ascontiguousarray(src_plane)
        ref_plane = np.ascontiguousarray(ref_plane)
        desc = np.ascontiguousarray(desc, dtype=np.int32).reshape(-1, 6)
        n = desc.shape[0]
        sad = np.zeros((n, NUM_SQ_PU), dtype=np.uint32)
        mv = np.zeros((n, NUM_SQ_PU), dtype=np.uint32)
        _check(lib().svthip_me_fullpel_search(self._h, src_plane.ctypes.data, src_plane.nbytes, src_plane.shape[1],
                                               ref_plane.ctypes.data, ref_plane.nbytes, ref_plane.shape[1],
                                               desc.ctypes.data, n, sad.ctypes.data, mv.ctypes.data))
        return sad, mv

    # -- device-pointer form (raw addresses, e.g. torch tensors' data_ptr()) -----------------------
    def fullpel_search_dev(self, d_src: int, src_stride: int, d_ref: int, ref_stride: int, d_desc: int, n_sb: int,
                           max_sw: int, max_sh: int, d_sad: int, d_mv: int, stream: int | None = None):
        _check(lib().svthip_me_fullpel_search_dev(self._h, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, max_sw,
                                                  max_sh, d_sad, d_mv, stream))

    def fullpel_search_time_dev(self, d_src: int, src_stride: int, d_ref: int, ref_stride: int, d_desc: int, n_sb: int,
                                max_sw: int, max_sh: int, d_sad: int, d_mv: int, iters: int) -> float:
        ms = C.c_float(0)
        _check(lib().svthip_me_fullpel_search_time_dev(self._h, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb,
                                                       max_sw, max_sh, d_sad, d_mv, iters, C.byref(ms)))
        return ms.value

    def fullpel_search209_dev(self, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, max_sw, max_sh, d_sad, d_mv, stream=None):
        """209-PU full-pel search (squares + rectangles); d_sad / d_mv: [n_sb][209] uint32 device arrays."""
        _check(lib().svthip_me_fullpel_search209_dev(self._h, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, max_sw, max_sh, d_sad, d_mv,
                                                     stream))

    def hme_search_center_dev(self, d_pool, cur, ref, params, list_index, d_sb, n_sb, d_l0_mv64, d_desc, d_center=None,
                              d_state=None, stream=None, l0_mv_stride=1):
        """cur/ref: PaPictureDesc, params: MeParams (host structs); the rest are device addresses."""
        _check(lib().svthip_me_hme_search_center_dev(self._h, d_pool, C.byref(cur), C.byref(ref), C.byref(params), list_index,
                                                     d_sb, n_sb, d_l0_mv64, l0_mv_stride, d_desc, d_center, d_state, stream))

    def hme_search_center_batch_dev(self, d_pool, curs, refs, params, list_index, d_sb, n_sb, d_l0_mv64, d_desc, d_center=None,
                                    d_state=None, stream=None, l0_mv_stride=1):
        """curs/refs: sequences of PaPictureDesc (one pair per job); per-SB device arrays hold the jobs back to back."""
        n = len(curs)
        ca = (PaPictureDesc * n)(*curs)
        ra = (PaPictureDesc * n)(*refs)
        _check(lib().svthip_me_hme_search_center_batch_dev(self._h, d_pool, ca, ra, n, C.byref(params), list_index, d_sb, n_sb, d_l0_mv64,
                                                           l0_mv_stride, d_desc, d_center, d_state, stream))

    def subpel_refine_dev(self, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, max_sw, max_sh, d_sad, d_mv, disable_8x8=False,
                          stream=None):
        _check(lib().svthip_me_subpel_refine_dev(self._h, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, max_sw, max_sh,
                                                 int(disable_8x8), d_sad, d_mv, stream))

    def subpel_refine209_dev(self, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, max_sw, max_sh, d_sad, d_mv, disable_8x8=False,
                             stream=None):
        """Sub-pel refinement of all 209 PUs; d_sad / d_mv: [n_sb][209] uint32 device arrays (ME-buffer order), in place."""
        _check(lib().svthip_me_subpel_refine209_dev(self._h, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, max_sw, max_sh,
                                                    int(disable_8x8), d_sad, d_mv, stream))

    def subpel_search_dev(self, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, max_sw, max_sh, d_sad, d_mv, method, all_pu,
                          disable_8x8=False, stream=None):
        """The refinement under one of the reference's fractional search methods; d_sad / d_mv: [n_sb][209 if all_pu else 85], in place."""
        _check(lib().svthip_me_subpel_search_dev(self._h, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, max_sw, max_sh,
                                                 int(disable_8x8), int(all_pu), int(method), d_sad, d_mv, stream))

    def bipred_pack_dev(self, d_src, src_stride, d_ref0, ref0_stride, d_desc0, d_ref1, ref1_stride, d_desc1, n_sb, max_sw, max_sh,
                        d_sad0, d_mv0, d_sad1, d_mv1, n_lists, d_out, bipred_8x8=True, stream=None):
        _check(lib().svthip_me_bipred_pack_dev(self._h, d_src, src_stride, d_ref0, ref0_stride, d_desc0, d_ref1, ref1_stride, d_desc1,
                                               n_sb, max_sw, max_sh, d_sad0, d_mv0, d_sad1, d_mv1, n_lists, int(bipred_8x8), d_out,
                                               stream))

    def bipred_pack209_dev(self, d_src, src_stride, d_ref0, ref0_stride, d_desc0, d_ref1, ref1_stride, d_desc1, n_sb, max_sw, max_sh,
                           d_sad0, d_mv0, d_sad1, d_mv1, n_lists, d_out, stream=None):
        """Bi-prediction + packing over all 209 PUs; d_out: [n_sb][209] ME_CU_RESULT_DTYPE in raster PU order."""
        _check(lib().svthip_me_bipred_pack209_dev(self._h, d_src, src_stride, d_ref0, ref0_stride, d_desc0, d_ref1, ref1_stride, d_desc1,
                                                  n_sb, max_sw, max_sh, d_sad0, d_mv0, d_sad1, d_mv1, n_lists, d_out, stream))

    def motion_estimate_picture_dev(self, d_pool, cur, ref0, ref1, params, d_sb, n_sb, d_out, use_subpel=True, cu8x8_mode=0,
                                    d_list_sad=None, d_list_mv=None, stream=None):
        """Whole-picture ME (MotionEstimateLcu over all SBs): ref1=None for P pictures."""
        _check(lib().svthip_motion_estimate_picture_dev(self._h, d_pool, C.byref(cur), C.byref(ref0),
                                                        C.byref(ref1) if ref1 is not None else None, C.byref(params),
                                                        int(use_subpel), int(cu8x8_mode), d_sb, n_sb, d_out, d_list_sad, d_list_mv,
                                                        stream))

    def motion_estimate_batch_dev(self, d_pool, curs, refs0, refs1, params, d_sb, n_sb, d_out, use_subpel=True, cu8x8_mode=0,
                                  d_list_sad=None, d_list_mv=None, stream=None):
        """Whole-picture ME of len(curs) pictures in one call; refs1=None for P pictures."""
        n = len(curs)
        ca, r0 = (PaPictureDesc * n)(*curs), (PaPictureDesc * n)(*refs0)
        r1 = (PaPictureDesc * n)(*refs1) if refs1 is not None else None
        _check(lib().svthip_motion_estimate_batch_dev(self._h, d_pool, ca, r0, r1, n, C.byref(params), int(use_subpel), int(cu8x8_mode),
                                                      d_sb, n_sb, d_out, d_list_sad, d_list_mv, stream))

    def motion_estimate209_batch_dev(self, d_pool, curs, refs0, refs1, params, d_sb, n_sb, d_out, use_subpel=True, cu8x8_mode=0,
                                     d_list_sad=None, d_list_mv=None, stream=None):
        """Whole-picture ME in the 209-PU mode of len(curs) pictures in one call; refs1=None for P pictures."""
        n = len(curs)
        ca, r0 = (PaPictureDesc * n)(*curs), (PaPictureDesc * n)(*refs0)
        r1 = (PaPictureDesc * n)(*refs1) if refs1 is not None else None
        _check(lib().svthip_motion_estimate209_batch_dev(self._h, d_pool, ca, r0, r1, n, C.byref(params), int(use_subpel), int(cu8x8_mode),
                                                         d_sb, n_sb, d_out, d_list_sad, d_list_mv, stream))

    def sad_loop_batch_dev(self, d_src, src_stride, d_ref, ref_stride, ref_stride_raw, d_desc, n_blocks, width, height, sw, sh, d_best_sad, d_best_xy,
                           stream=None):
        """SadLoopKernel over n_blocks (src_offset, ref_offset) uint32 pairs; d_best_sad uint32 [n], d_best_xy int16 [n][2] = (x, y) index."""
        _check(lib().svthip_sad_loop_batch_dev(self._h, d_src, src_stride, d_ref, ref_stride, ref_stride_raw, d_desc, n_blocks, width, height, sw, sh,
                                               d_best_sad, d_best_xy, stream))

    # -- in-loop motion estimation (849 blocks per 64x64 superblock, one list per call) ---------------
    def inloop_centers_dev(self, d_me, me_pu_stride, list_index, n_sb, d_center, stream=None):
        """d_me: [n_sb][me_pu_stride] ME_CU_RESULT_DTYPE rows -> d_center int16 [n_sb][2], the 64x64 block's vector of the list >> 2."""
        _check(lib().svthip_me_inloop_centers_dev(self._h, d_me, me_pu_stride, list_index, n_sb, d_center, stream))

    def inloop_area_dev(self, d_center, d_sb, n_sb, pic_width, pic_height, src_geom, ref_geom, area_w, area_h, d_desc, stream=None):
        """src_geom / ref_geom: (stride, origin_x, origin_y) of the planes -> d_desc [n_sb] INLOOP_DESC_DTYPE."""
        _check(lib().svthip_me_inloop_area_dev(self._h, d_center, d_sb, n_sb, pic_width, pic_height, *src_geom, *ref_geom, area_w, area_h, d_desc, stream))

    def inloop_fullpel_search_dev(self, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, block_set, d_sad, d_mv, stream=None):
        """d_sad / d_mv: [n_sb][849] uint32 in the reference's buffer order; INLOOP_BLOCKS_SIDE_4 leaves the other 209 slots untouched."""
        _check(lib().svthip_me_inloop_fullpel_search_dev(self._h, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, int(block_set), d_sad, d_mv, stream))

    def inloop_subpel_search_dev(self, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, block_set, d_sad, d_mv, stream=None):
        """Half-pel and quarter-pel refinement of the full-pel results, in place; same arguments as inloop_fullpel_search_dev."""
        _check(lib().svthip_me_inloop_subpel_search_dev(self._h, d_src, src_stride, d_ref, ref_stride, d_desc, n_sb, int(block_set), d_sad, d_mv, stream))

    def inloop_pack_dev(self, d_mv, n_sb, d_inloop_mv, stream=None):
        """d_mv [n_sb][849] uint32 -> d_inloop_mv int16 [n_sb][849][2], x then y, in the candidate order of inloop_me_mv."""
        _check(lib().svthip_me_inloop_pack_dev(self._h, d_mv, n_sb, d_inloop_mv, stream))

    def inloop_search_dev(self, d_src, src_geom, d_ref, ref_geom, pic_width, pic_height, d_center, d_sb, n_sb, area_w, area_h, d_sad, d_mv,
                          d_inloop_mv, use_subpel=False, block_set=0, stream=None):
        """Areas, full-pel search, sub-pel refinement if asked for, and reorder of one list in one call; src_geom / ref_geom: (stride, origin_x, origin_y)."""
        _check(lib().svthip_me_inloop_search_dev(self._h, d_src, *src_geom, d_ref, *ref_geom, pic_width, pic_height, d_center, d_sb, n_sb, area_w, area_h,
                                                 int(use_subpel), int(block_set), d_sad, d_mv, d_inloop_mv, stream))
