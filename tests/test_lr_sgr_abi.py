"""The self-guided loop-restoration entries are declared in include/svtav1_hip.h, exported by the library, bound by the package, and the
restatement's record is the package's (no GPU needed; every size, offset and #define is held to the compiler's by
tests/test_binding_vs_header.py)."""
import ctypes
import os
import re
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ENTRIES = ("svthip_sgrproj_workspace_bytes", "svthip_sgrproj_walk_max_trials", "svthip_av1_selfguided_restoration_dev",
           "svthip_av1_highbd_selfguided_restoration_dev", "svthip_sgrproj_solve_dev", "svthip_sgrproj_walk_table_dev", "svthip_av1_search_sgrproj_dev",
           "svthip_av1_highbd_search_sgrproj_dev", "svthip_av1_sgrproj_trial_sse_dev", "svthip_av1_highbd_sgrproj_trial_sse_dev",
           "svthip_av1_lr_filter_frame_dev", "svthip_av1_highbd_lr_filter_frame_dev")
METHODS = ("av1_selfguided_restoration_dev", "sgrproj_solve_dev", "sgrproj_walk_table_dev", "av1_search_sgrproj_dev", "av1_sgrproj_trial_sse_dev",
           "av1_lr_filter_frame_dev")


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
    assert "struct svthip_sgrproj_detail" in text


def test_header_compiles_as_c99_and_the_record_matches_the_binding():
    import lr_sgr_util as su
    import svtav1_hip
    assert su.DETAIL_DTYPE is svtav1_hip.SGRPROJ_DETAIL_DTYPE


def test_host_functions_of_the_library():
    """no device: the walk's bound is the restatement's, and the workspace holds 64 bytes per sample plus the per-(unit, set) records"""
    import lr_sgr_util as su
    import lr_util as lu
    import svtav1_hip
    assert svtav1_hip.sgrproj_walk_max_trials() == su.max_walk_trials() == 131
    for (w, h) in ((64, 64), (200, 136), (1920, 1080)):
        samples = w * h * 3 // 2
        n = svtav1_hip.sgrproj_workspace_bytes(w, h)
        most_jobs = 3 * lu.units_in(w, 64) * lu.units_in(h, 64) * 16          # unit size 64 in every plane
        assert samples * 64 + svtav1_hip.lr_unit_geometry(w, h)[0][3] * 16 * 80 <= n <= samples * 64 + most_jobs * 96 + 4096
