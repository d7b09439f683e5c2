"""The restoration-decision entries are declared in include/svtav1_hip.h, exported by the library and bound by the package; the two
structs have their stated sizes (every size, offset and #define is held to the compiler's by tests/test_binding_vs_header.py); the workspace of the one-call entry holds both searches'
workspaces (no GPU needed)."""
import ctypes
import os
import re
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ENTRIES = ("svthip_rest_finish_search_dev", "svthip_av1_pick_filter_restoration_dev", "svthip_av1_highbd_pick_filter_restoration_dev",
           "svthip_lr_pick_workspace_bytes")
METHODS = ("rest_finish_search_dev", "av1_pick_filter_restoration_dev")


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
    assert callable(svtav1_hip.lr_pick_workspace_bytes)
    assert "struct svthip_rest_finish_rates" in text and "struct svthip_rest_finish_result" in text
    assert svtav1_hip.RESTORE_SWITCHABLE == 3 and re.search(r"#define SVTHIP_RESTORE_SWITCHABLE 3\b", text)
    # the gap is closed in the header's own words
    assert not re.search(r"staying on the host:[^.]*rest_finish_search", open(os.path.join(ROOT, "include", "svtav1_hip.h")).read())


def test_header_compiles_as_c99_and_the_structs_match_the_dtype_functions():
    import abi_util
    import svtav1_hip
    abi_util.assert_sizes((svtav1_hip.rest_finish_rates_dtype(), 32), (svtav1_hip.rest_finish_result_dtype(), 104))
    assert svtav1_hip.rest_finish_rates_dtype().names == ("rdmult", "wiener_cost", "sgrproj_cost", "switchable_cost")


def test_workspace_of_the_one_call_entry():
    import svtav1_hip
    for (w, h) in ((64, 64), (200, 200), (1920, 1080), (3840, 2160)):
        for us in (None, (64, 64, 64)):
            n = svtav1_hip.lr_unit_geometry(w, h, us)[0][3]
            both = svtav1_hip.lr_workspace_bytes(n) + svtav1_hip.sgrproj_workspace_bytes(w, h)
            got = svtav1_hip.lr_pick_workspace_bytes(w, h, us)
            assert both + n * 28 + 4 <= got <= both + n * 28 + 8 * 256, (w, h, us, got, both)     # wiener_sse, sgr_sse, n_trials, pending
    for bad in ((0, 64, None), (64, 0, None), (60, 64, None), (64, 64, (64, 64, 32)), (64, 64, (100, 64, 64)), (16392, 64, None)):
        assert svtav1_hip.lr_pick_workspace_bytes(*bad) == 0, bad
