"""CPU: the full-loop entries in the library and the header -- the symbols, and the sizes of svthip_md_full_desc / _result / _decision, without
padding, as the md_full_*_dtype() functions of the package give them (every size, offset and #define is held to the compiler's by
tests/test_binding_vs_header.py)."""
import os

import numpy as np

import abi_util
import svtav1_hip
from svtav1_hip import _abi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LAYOUTS = (("svthip_md_full_desc", svtav1_hip.md_full_desc_dtype, 48), ("svthip_md_full_result", svtav1_hip.md_full_result_dtype, 144),
           ("svthip_md_full_decision", svtav1_hip.md_full_decision_dtype, 16))
CONSTANTS = {"MD_FULL_LUMA": "SVTHIP_MD_FULL_LUMA", "MD_FULL_CHROMA": "SVTHIP_MD_FULL_CHROMA", "MD_FULL_DECIDE": "SVTHIP_MD_FULL_DECIDE",
             "MD_FULL_MAX_SLOTS": "SVTHIP_MD_FULL_MAX_SLOTS"}


def test_symbols_are_exported_and_bound():
    lib = svtav1_hip.lib()
    for name, n_args in (("svthip_md_full_workspace_bytes", 6), ("svthip_md_full_loop_batch_dev", 27)):
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args, name
    assert svtav1_hip.lib().svthip_md_full_workspace_bytes.restype is not None
    assert hasattr(svtav1_hip.Context, "md_full_loop_batch_dev")


def test_header_is_c99_and_layouts_match():
    for cname, dtype, size in LAYOUTS:
        dt = dtype()
        assert isinstance(dt, np.dtype) and dt is _abi.dtype(cname, **({"lambda_": "lambda"} if "lambda_" in dt.names else {})) and size % 16 == 0
        abi_util.assert_sizes((dt, size))
        # every byte of the struct belongs to a field: no padding the dtype does not see
        assert sum(dt.fields[k][0].itemsize for k in dt.names) == size
    assert [getattr(svtav1_hip, k) for k in CONSTANTS] == [_abi.define(v) for v in CONSTANTS.values()] == [1, 2, 4, 12]


def test_workspace_bytes_follow_the_masks():
    w = svtav1_hip.md_full_workspace_bytes
    none, m0 = w(10, 4, 8, 8, 1, 1), w(10, 4, 8, 8, svtav1_hip.tx_search_type_mask(1, 1, 0, 0), svtav1_hip.tx_search_type_mask(1, 0, 0, 0))
    assert 0 < none < m0 and none % 16 == 0 and m0 % 16 == 0
    assert w(20, 4, 8, 8, 1, 1) > none and w(10, 8, 8, 8, 1, 1) > none and w(0, 4, 8, 8, 1, 1) >= 0
    assert w(10, 4, 8, 8, 0, 1) == 0 and w(10, 4, 8, 8, 1, 0x10000) == 0 and w(10, 4, 64, 64, 0x3, 1) == 0
