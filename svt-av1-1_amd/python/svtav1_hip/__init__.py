"""ctypes binding of libsvtav1_hip.so (the C ABI in include/svtav1_hip.h) for tests and bench.py.

The product is the shared library; this package only marshals numpy / torch device pointers into it.
There is no Python or CPU fallback: if the library is missing, import of `lib()` raises.

Signatures, struct layouts and the constants that mirror a #define all come from the header (_abi).  One module per family of the header
names its descriptors, dtypes and constants and holds its helpers and the Context methods of that family; everything public is
re-exported here.
"""
from __future__ import annotations

from ._core import (LIB_PATH, OPT_CONVOLVE_VALU, OPT_SADLOOP_GENERIC, OPT_TQ_MAX_WORKGROUPS, ContextCore, SvtHipError, lib, u8p,
                    u32p)
from ._me import (FRACTIONAL_FULL_SAD_SEARCH, FRACTIONAL_SSD_SEARCH, FRACTIONAL_SUB_SAD_SEARCH, HME_LEVEL0_MULTIPLIER, HME_MAX_JOBS,
                  INLOOP_BLOCKS_ALL, INLOOP_BLOCKS_SIDE_4, INLOOP_DESC_DTYPE, INLOOP_ME_PU_COUNT, InloopDesc, MAX_SAD_VALUE,
                  ME_CU_RESULT_DTYPE, NUM_SQ_PU, FullpelDesc, MeCuResult, MeParams, MotionEstimation, PaPictureDesc, SbOrigin,
                  build_picture_pool, default_me_params, make_fullpel_desc, sb_origins, shard_sb_rows)
from ._tq import (COEFF_RATE_DESC_DTYPE, COEFF_RATE_TABLES_DTYPE, ITXFM_DESC_DTYPE, LV_MAP_COEFF_COST_DTYPE, QUANT_DESC_DTYPE,
                  TU_DESC_DTYPE, TU_RECON_SCRATCH, TX_SIZES_WH, TXFM_DESC_DTYPE, TransformQuant, TuBatcher, TuResult, TxSearchResult,
                  TxSearchTu, tx_search_type_mask, valid_tx_types)
from ._analysis import SSE_SRC_16BIT, SSE_SRC_COMPRESSED, SSE_SRC_UNPACKED, OisParams, PictureAnalysis, make_planes
from ._pred import (AV1_BLOCK_SIZES_WH, BI_PRED, CONVOLVE_COMPOUND_DESC_DTYPE, CONVOLVE_DESC_DTYPE, INTER_PU_DESC_DTYPE, INTRA_DESC_DTYPE,
                    UNI_PRED_LIST_0, UNI_PRED_LIST_1, WARP_AFFINE, WARP_BLOCK_SIZES_WH, WARP_PU_DESC_DTYPE, WARP_ROTZOOM, InterPlanes,
                    Prediction)
from ._cfl import CFL_DECISION_DTYPE, CFL_DECISION_JOB_DTYPE, CFL_DESC_DTYPE, CFL_LUMA_SIZES_WH, Cfl
from ._deblock import LF_MI_DTYPE, Deblocking, LfPicture, make_lf_picture
from ._cdef import CDEF_PICK_MAX_FB, CDEF_RESULT_DTYPE, Cdef, CdefPicture, cdef_filter_blocks, cdef_search128_workspace_bytes, make_cdef_picture
from ._restoration import (RESTORE_NONE, RESTORE_SGRPROJ, RESTORE_SWITCHABLE, RESTORE_WIENER, SGRPROJ_DETAIL_DTYPE, SGRPROJ_PARAMS,
                           WIENER_WALK_STATE_DTYPE, LrPicture, Restoration, lr_pick_workspace_bytes, lr_unit_geometry, lr_unit_sizes,
                           lr_workspace_bytes, make_lr_picture, rest_finish_rates_dtype, rest_finish_result_dtype, sgrproj_walk_max_trials,
                           sgrproj_workspace_bytes, wiener_walk_max_trials)
from ._grain import (FILM_GRAIN_FLAT_TABLES_DOUBLES, FILM_GRAIN_NOISE_BLOCK_SIZE, FILM_GRAIN_NOISE_INSUFFICIENT_FLAT_BLOCKS,
                     FILM_GRAIN_NOISE_INTERNAL_ERROR, FILM_GRAIN_NOISE_LAG, FILM_GRAIN_NOISE_OK, FILM_GRAIN_NOISE_SHAPE_SQUARE, FILM_GRAIN_PARAMS_BYTES,
                     FILM_GRAIN_TABLES_BYTES, FilmGrain, film_grain_flat_block_features_dtype, film_grain_noise_state_dtype, film_grain_noise_psd_default, film_grain_param_offsets,
                     film_grain_params, film_grain_wiener_workspace_bytes)
from ._md import (MD_FAST_CHROMA_QUARTER, MD_FAST_INVALID, MD_FAST_LUMA_GIVEN, MD_FAST_MAX_BUFFERS, MD_FAST_MAX_CANDIDATES, MD_FAST_SKIP_DISTORTION,
                  MD_FAST_TYPE_INTER, MD_IFS_REFUSED, MD_IFS_SEARCH_FAST, MD_IFS_SEARCH_FULL, InterpFilterSearch, ModeDecisionFast, md_fast_desc_dtype,
                  md_fast_group_dtype, md_fast_pick_dtype, md_fast_result_dtype, md_ifs_desc_dtype, md_ifs_result_dtype, md_model_rd_desc_dtype,
                  md_model_rd_result_dtype)
from ._md import (MD_FULL_CHROMA, MD_FULL_DECIDE, MD_FULL_LUMA, MD_FULL_MAX_SLOTS, MD_FULL_NONE, ModeDecisionFull, md_full_decision_dtype,
                  md_full_desc_dtype, md_full_result_dtype, md_full_workspace_bytes, md_full128_tu_dtype, md_full128_workspace_bytes)
from ._md import (MD_PART_BLOCKS_64, MD_PART_BLOCKS_128, MD_PART_MAX_FINAL_64, MD_PART_MAX_FINAL_128, MD_PART_MDC_SPLIT_FLAG, MD_PART_NONE,
                  MD_PART_SPLIT_FLAG, MD_PART_TESTED, ModeDecisionPartition, md_partition_block_dtype, md_partition_final_dtype, md_partition_geometry,
                  md_partition_leaf_dtype, md_partition_result_dtype, md_partition_sb_dtype)
from ._host import ME_CU_RESULT_REF_DTYPE, HostForms, HostPicture
from ._ma import MA_PICTURE_PARAMS_DTYPE, MaPictureParams, MotionAnalysis, make_ma_params


class Context(ContextCore, MotionEstimation, TransformQuant, PictureAnalysis, Prediction, Cfl, Deblocking, Cdef, Restoration, FilmGrain, ModeDecisionFast, InterpFilterSearch, ModeDecisionFull, ModeDecisionPartition, HostForms, MotionAnalysis):
    """One svthip_ctx (stream + scratch), the analogue of one MeContext_t."""
