"""The fast-loop entries are declared in include/svtav1_hip.h, exported by the library and bound by the package; the structs have the sizes the
restatement assumes and the flags its values (no GPU needed; the compiler's sizes, offsets and constants are held for every struct and #define by tests/test_binding_vs_header.py)."""
import ctypes
import os
import re
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ENTRIES = ("svthip_md_fast_cost_batch_dev", "svthip_md_fast_pick_batch_dev")
METHODS = ("md_fast_cost_batch_dev", "md_fast_pick_batch_dev")


def test_header_declares_library_exports_and_package_binds_every_entry():
    import svtav1_hip
    full = open(os.path.join(ROOT, "include", "svtav1_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    declared = set(re.findall(r"\b(svthip_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(svtav1_hip.LIB_PATH)
    for n in ENTRIES:
        assert n in declared, f"{n} is not declared in include/svtav1_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert getattr(svtav1_hip.lib(), n).argtypes is not None, f"{n} has no argument types in the binding"
    assert len(svtav1_hip.lib().svthip_md_fast_cost_batch_dev.argtypes) == 9 and len(svtav1_hip.lib().svthip_md_fast_pick_batch_dev.argtypes) == 8
    for m in METHODS:
        assert callable(getattr(svtav1_hip.Context, m, None)), m
    for s in ("svthip_md_fast_desc", "svthip_md_fast_result", "svthip_md_fast_group", "svthip_md_fast_pick"):
        assert f"struct {s}" in text
    # the section cites the reference lines it replaces
    section = full[full.index("Mode decision's fast loop"):full.index("svthip_md_fast_cost_batch_dev(")]
    for cite in ("EbProductCodingLoop.c:1282-1459", "EbModeDecision.c:393-471", "EbRateDistortionCost.c:764-771", ":1321-1343"):
        assert cite in section, cite


def test_header_compiles_as_c99_and_the_structs_match_the_binding():
    import abi_util
    import md_fast_util as mu
    import svtav1_hip
    abi_util.assert_sizes((svtav1_hip.md_fast_desc_dtype(), 32), (svtav1_hip.md_fast_result_dtype(), 16), (svtav1_hip.md_fast_group_dtype(), 8),
                          (svtav1_hip.md_fast_pick_dtype(), 32))
    flags = {"LUMA_GIVEN": mu.LUMA_GIVEN, "SKIP_DISTORTION": mu.SKIP_DISTORTION, "INVALID": mu.INVALID, "CHROMA_QUARTER": mu.CHROMA_QUARTER,
             "TYPE_INTER": mu.TYPE_INTER, "MAX_CANDIDATES": mu.MAX_CANDIDATES, "MAX_BUFFERS": mu.MAX_BUFFERS}
    for k, v in flags.items():
        assert getattr(svtav1_hip, f"MD_FAST_{k}") == v
