"""The six in-loop motion estimation entries are declared in include/svtav1_hip.h, exported by the library and bound by the package;
svthip_inloop_desc has the size and offsets the C compiler gives it; the constants have the values the header states (no GPU needed)."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import abi_util  # noqa: E402,F401

ENTRIES = {"svthip_me_inloop_centers_dev": 7, "svthip_me_inloop_area_dev": 16, "svthip_me_inloop_fullpel_search_dev": 11, "svthip_me_inloop_subpel_search_dev": 11, "svthip_me_inloop_pack_dev": 5,
           "svthip_me_inloop_search_dev": 22}
METHODS = ("inloop_centers_dev", "inloop_area_dev", "inloop_fullpel_search_dev", "inloop_subpel_search_dev", "inloop_pack_dev", "inloop_search_dev")
FIELDS = ("src_offset", "ref_offset", "x_search_area_origin", "y_search_area_origin", "search_area_width", "search_area_height", "sb_width", "sb_height")


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
    # the section cites the reference lines it replaces, says how the reference ships and what is left out
    section = full[full.index("In-loop motion estimation: the second motion search"):full.index("svthip_me_inloop_search_dev(")]
    for cite in ("EbProductCodingLoop.c:6300-6733", "EbEncDecProcess.c:1502-1580", "DISABLE_IN_LOOP_ME 1", "EbDefinitions.h:129", ":2894-2917", ":3025-3528",
                 ":3605-3878", ":3884-3911", ":6389-6452", ":6626-6728", ":4007-4094", ":4304-4984", ":5320-5990", "Left out", "128x128", "USE_INLOOP_ME_FULL_SAD", "get_in_loop_me_info_index",
                 ":6456-6480", "63 samples", "tab4x16"):
        assert cite in section, cite


def test_constants_and_descriptor_layout_match_the_compiler(tmp_path):
    import svtav1_hip
    assert (svtav1_hip.INLOOP_ME_PU_COUNT, svtav1_hip.INLOOP_BLOCKS_ALL, svtav1_hip.INLOOP_BLOCKS_SIDE_4) == (849, 0, 1)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svtav1_hip.h"\nint main(void) {\n  printf("%zu", sizeof(svthip_inloop_desc));\n' +
                   "".join(f'  printf(" %zu", offsetof(svthip_inloop_desc, {f}));\n' for f in FIELDS) +
                   '  printf(" %d %d %d\\n", SVTHIP_INLOOP_ME_PU_COUNT, SVTHIP_INLOOP_BLOCKS_ALL, SVTHIP_INLOOP_BLOCKS_SIDE_4);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [32] + [4 * i for i in range(8)] + [849, 0, 1]
    dt = svtav1_hip.INLOOP_DESC_DTYPE
    assert dt.itemsize == ctypes.sizeof(svtav1_hip.InloopDesc) == 32 and dt.names == FIELDS
    assert [dt.fields[f][1] for f in FIELDS] == [4 * i for i in range(8)]
