"""The CDEF entries are declared in include/svtav1_hip.h, exported by the library and bound by the package; the restatement's result record is the
package's (every size, offset and #define is held to the compiler's by tests/test_binding_vs_header.py); the quantiser table behind lambda is the project's pinned one (no GPU needed)."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ENTRIES = ("svthip_av1_cdef_search_mse_dev", "svthip_av1_highbd_cdef_search_mse_dev", "svthip_cdef_pick_strengths_dev", "svthip_av1_cdef_search_dev",
           "svthip_av1_highbd_cdef_search_dev", "svthip_av1_cdef_frame_dev", "svthip_av1_highbd_cdef_frame_dev", "svthip_cdef_dist_8x8_batch_dev")
METHODS = ("av1_cdef_search_mse_dev", "cdef_pick_strengths_dev", "av1_cdef_search_dev", "av1_cdef_frame_dev", "cdef_dist_8x8_batch_dev")


def test_header_declares_library_exports_and_package_binds_every_entry():
    import svtav1_hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svtav1_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(svthip_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(svtav1_hip.LIB_PATH)
    for n in ENTRIES:
        assert n in declared, f"{n} is not declared in include/svtav1_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert getattr(svtav1_hip.lib(), n).argtypes is not None, f"{n} has no argument types in the binding"
    for m in METHODS:
        assert callable(getattr(svtav1_hip.Context, m, None)), m
    assert "struct svthip_cdef_picture" in text and "struct svthip_cdef_result" in text
    # the section sits after the loop-filter one and before loop restoration
    full = open(os.path.join(ROOT, "include", "svtav1_hip.h")).read()
    assert full.index("svthip_av1_highbd_pick_filter_level_dev(") < full.index("svthip_av1_cdef_search_mse_dev(") < full.index("svthip_av1_wiener_stats_dev(")


def test_header_compiles_as_c99_and_the_structs_match_the_binding():
    import cdef_util as cu
    import svtav1_hip
    from svtav1_hip import _abi
    assert cu.RESULT_DTYPE is svtav1_hip.CDEF_RESULT_DTYPE
    assert svtav1_hip.CDEF_PICK_MAX_FB == 4096 and _abi.define("SVTHIP_CDEF_STRENGTHS") == 64


def test_quantiser_table_behind_lambda_is_the_pinned_one():
    """svt-av1-1_amd/csrc/cf_cdef_ac_quant.inc (tools/gen_cdef_ac_quant.py) holds dequant[1] of the luma rows of tests/golden/quant_tables.npz"""
    import svtav1_hip
    text = open(os.path.join(ROOT, "svt-av1-1_amd", "csrc", "cf_cdef_ac_quant.inc")).read()
    rows = [list(map(int, re.findall(r"\d+", row))) for row in re.findall(r"\{([^{}]+)\}", text)]
    z = np.load(os.path.join(ROOT, "tests", "golden", "quant_tables.npz"))
    assert len(rows) == 2
    for row, bd in zip(rows, (8, 10)):
        assert row == [int(v) for v in z[f"rows_bd{bd}_inter"][:, 0, 9]]
    assert svtav1_hip.cdef_filter_blocks(200, 136) == (4, 3) and svtav1_hip.cdef_filter_blocks(1920, 1080) == (30, 17)
