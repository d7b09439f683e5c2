"""The interpolation-filter search entries are declared in include/svtav1_hip.h, exported by the library and bound by the package; the
structs have the sizes the restatement assumes (no GPU needed; every size, offset and #define is held to the compiler's by
tests/test_binding_vs_header.py)."""
import ctypes
import os
import re
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ENTRIES = {"svthip_md_model_rd_batch_dev": 10, "svthip_md_interp_filter_search_batch_dev": 15}
METHODS = ("md_model_rd_batch_dev", "md_interp_filter_search_batch_dev")


def test_header_declares_library_exports_and_package_binds_every_entry():
    import svtav1_hip
    full = open(os.path.join(ROOT, "include", "svtav1_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    declared = set(re.findall(r"\b(svthip_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(svtav1_hip.LIB_PATH)
    for n, n_args in ENTRIES.items():
        assert n in declared, f"{n} is not declared in include/svtav1_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert len(getattr(svtav1_hip.lib(), n).argtypes) == n_args, f"{n}: argument count in the binding"
    # quantizer, the reference's int16_t, crosses the ABI as an int32_t (the binding's scalar table has no 16-bit signed type)
    assert svtav1_hip.lib().svthip_md_model_rd_batch_dev.argtypes[7] is ctypes.c_int32
    assert svtav1_hip.lib().svthip_md_interp_filter_search_batch_dev.argtypes[11] is ctypes.c_int32
    for m in METHODS:
        assert callable(getattr(svtav1_hip.Context, m, None)), m
    for s in ("svthip_md_model_rd_desc", "svthip_md_model_rd_result", "svthip_md_ifs_desc", "svthip_md_ifs_result"):
        assert f"struct {s}" in text
    # the section cites the reference lines it replaces, and says which dir is the x filter
    section = full[full.index("Mode decision's interpolation-filter search"):full.index("svthip_md_model_rd_batch_dev(svthip_ctx")]
    for cite in ("EbInterPrediction.c:3523-3854", ":4327-4366", "EbPictureDecisionProcess.c:385-388", ":3378-3468", ":3161-3190", ":3339-3376", ":3314-3337",
                 ":3248-3312", ":3241-3244", ":3114-3151", ":3511-3515", ":3615-3764", ":3765-3837", ":3630-3631", "convolve.h:31-34",
                 "dir 1 the HORIZONTAL (x) filter"):
        assert cite in section, cite


def test_header_compiles_as_c99_and_the_structs_match_the_binding():
    import abi_util
    import md_ifs_util as mu
    import svtav1_hip
    abi_util.assert_sizes((svtav1_hip.md_model_rd_desc_dtype(), 16), (svtav1_hip.md_model_rd_result_dtype(), 32), (svtav1_hip.md_ifs_desc_dtype(), 32),
                          (svtav1_hip.md_ifs_result_dtype(), 32))
    filter_rate = svtav1_hip.md_ifs_desc_dtype()["filter_rate"]
    assert filter_rate.itemsize == 24 and filter_rate.shape == (2, 3) and filter_rate.base.itemsize == 4   # rows of 12 bytes
    assert (svtav1_hip.MD_IFS_SEARCH_FAST, svtav1_hip.MD_IFS_SEARCH_FULL, svtav1_hip.MD_IFS_REFUSED) == (1, 2, mu.REFUSED)
