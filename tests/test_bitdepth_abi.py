"""The five entries of the 10-bit picture forms are declared in include/svtav1_hip.h, exported by the library and bound by the package; 
svthip_planes has 40 bytes and the source forms their values (no GPU needed; every size, offset and #define is held to the compiler's by
tests/test_binding_vs_header.py)."""
import ctypes
import os
import re
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ENTRIES = {"svthip_pa_unpack_10bit_dev": 11, "svthip_pa_pack_10bit_dev": 11, "svthip_pa_pack_10bit_compressed_dev": 11, "svthip_picture_sse_dev": 10,
           "svthip_highbd_picture_sse_dev": 13}
METHODS = ("pa_unpack_10bit_dev", "pa_pack_10bit_dev", "picture_sse_dev", "highbd_picture_sse_dev")


def test_header_declares_library_exports_and_package_binds_every_entry():
    import svtav1_hip
    full = open(os.path.join(ROOT, "include", "svtav1_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    declared = set(re.findall(r"\b(svthip_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(svtav1_hip.LIB_PATH)
    for n, n_args in ENTRIES.items():
        assert n in declared, f"{n} is not declared in include/svtav1_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        fn = getattr(svtav1_hip.lib(), n)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args and fn.restype is ctypes.c_int32, n
    for m in METHODS:
        assert callable(getattr(svtav1_hip.Context, m, None)), m
    assert "struct svthip_planes" in text
    # the section cites the reference lines it replaces and states the compressed layout
    section = full[full.index("The 10-bit picture forms"):full.index("svthip_highbd_picture_sse_dev(")]
    for cite in ("EbPackUnPack_C.c:127-151", ":152-174", "EbEncHandle.c:2954-2985", "EbPackUnPack_C.c:12-38", "EbCodingLoop.c:2941-2974", ":2955-2957",
                 "EbPackUnPack_C.c:44-86", "EbCodingLoop.c:2888-2929", "EbInterPrediction.c:1447-1473", "EbEncDecProcess.c:775-1133", ":858-860",
                 ":1129-1131", "sb_y * (pw / 4) + (sb_x / 4) * sb_h", "bits 7..6", "uint32_t"):
        assert cite in section, cite


def test_header_compiles_as_c99_and_svthip_planes_matches_the_binding():
    import svtav1_hip
    p = svtav1_hip.make_planes([1, 2, 3], [4, 5, 6])
    t = type(p)
    assert ctypes.sizeof(t) == 40 and [int(v) for v in p.offset] == [1, 2, 3] and [int(v) for v in p.stride] == [4, 5, 6]
    assert (svtav1_hip.SSE_SRC_16BIT, svtav1_hip.SSE_SRC_UNPACKED, svtav1_hip.SSE_SRC_COMPRESSED) == (0, 1, 2)
