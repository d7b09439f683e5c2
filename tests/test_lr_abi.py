"""The Wiener loop-restoration entries are declared in include/svtav1_hip.h, exported by the library, bound by the package, and the walk
state keeps its taps at byte 8 (no GPU needed; every size, offset and #define is held to the compiler's by tests/test_binding_vs_header.py)."""
import ctypes
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

ENTRIES = ("svthip_lr_unit_geometry", "svthip_lr_workspace_bytes", "svthip_wiener_walk_max_trials", "svthip_av1_wiener_stats_dev",
           "svthip_av1_highbd_wiener_stats_dev", "svthip_wiener_solve_dev", "svthip_av1_wiener_trial_sse_dev", "svthip_av1_highbd_wiener_trial_sse_dev",
           "svthip_wiener_walk_init_dev", "svthip_wiener_walk_step_dev", "svthip_av1_search_wiener_dev", "svthip_av1_highbd_search_wiener_dev",
           "svthip_av1_loop_restoration_filter_frame_dev", "svthip_av1_highbd_loop_restoration_filter_frame_dev")


def test_header_declares_and_library_exports_every_entry():
    import svtav1_hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svtav1_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(svthip_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(svtav1_hip.LIB_PATH)
    for n in ENTRIES:
        assert n in declared, f"{n} is not declared in include/svtav1_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
    assert "struct svthip_lr_picture" in text and "struct svthip_wiener_walk_state" in text


def test_header_compiles_as_c99_and_layouts_match_the_binding():
    import svtav1_hip
    assert svtav1_hip.WIENER_WALK_STATE_DTYPE.fields["taps"][1] == 8


def test_geometry_and_walk_bound_from_the_library():
    """host functions of the library, no device: the geometry the kernels launch with and the default step count"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np

    import lr_util as lu
    import svtav1_hip
    for (w, h) in ((64, 64), (200, 136), (136, 200), (392, 264), (1920, 1080), (352, 288), (360, 288), (8, 8), (96, 320), (4096, 2176)):
        base, limits = svtav1_hip.lr_unit_geometry(w, h)
        planes, want_base = lu.picture_units(w, h)
        assert base == want_base and np.array_equal(limits, np.concatenate([p[0] for p in planes])), (w, h)
    base, limits = svtav1_hip.lr_unit_geometry(200, 136, (64, 64, 64))
    planes, want_base = lu.picture_units(200, 136, (64, 64, 64))
    assert base == want_base and np.array_equal(limits, np.concatenate([p[0] for p in planes]))
    assert svtav1_hip.lr_unit_geometry(200, 132)[0] == [0, 0, 0, 0] and svtav1_hip.lr_unit_geometry(200, 136, (64, 96, 64))[0] == [0, 0, 0, 0]
    for win in (5, 7):
        assert svtav1_hip.wiener_walk_max_trials(win) == lu.max_walk_trials(win)
    assert svtav1_hip.wiener_walk_max_trials(7) == 81 and svtav1_hip.wiener_walk_max_trials(6) == 0
    assert svtav1_hip.lr_workspace_bytes(40) >= 40 * (1325 + 49 + 2401 + 2) * 8
