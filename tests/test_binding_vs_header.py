"""The Python package against include/svtav1_hip.h (no GPU needed): the signatures the package sets on the library are the header's, every
struct mirror has the C struct's size and offsets, every constant that mirrors a #define equals it, and the package's public surface is
the one recorded in tests/golden/binding_surface.json before the signatures were read from the header."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess
import tempfile
import types

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "svtav1_hip.h")
SCALAR_BYTES_SIGNED = {"int32_t": (4, True), "uint32_t": (4, False), "uint16_t": (2, False), "size_t": (C.sizeof(C.c_size_t), False)}


def _header_prototypes():
    """{name: (return declaration, [parameter declarations])}, read here a second time, independently of the package"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    out = {}
    for statement in text.split(";"):
        m = re.search(r"([^{}]*?)\b(svthip_[a-z0-9_]+)\s*\((.*)\)\s*$", statement, flags=re.S)
        if m:
            params = " ".join(m.group(3).split())
            out[m.group(2)] = (" ".join(m.group(1).split()), [] if params == "void" else [p.strip() for p in params.split(",")])
    return out


def _assert_is(ctype, decl, what):
    """a ctypes type against a C declaration: a pointer or array is c_void_p (const char * returns c_char_p), a scalar has the width and sign"""
    if "*" in decl or "[" in decl:
        assert ctype is (C.c_char_p if decl.startswith("const char *") and what.endswith("returns") else C.c_void_p), (what, decl, ctype)
        return
    size, signed = SCALAR_BYTES_SIGNED[[w for w in decl.split() if w != "const"][0]]
    assert ctype is not None and issubclass(ctype, C._SimpleCData) and ctype not in (C.c_void_p, C.c_char_p), (what, decl, ctype)
    assert C.sizeof(ctype) == size and (ctype(-1).value < 0) == signed, (what, decl, ctype)


def test_every_prototype_is_bound_with_the_headers_types():
    import svtav1_hip
    protos = _header_prototypes()
    assert len(protos) >= 114
    lib = svtav1_hip.lib()
    for name, (ret, params) in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, fn.argtypes, params)
        for i, (ctype, decl) in enumerate(zip(fn.argtypes, params)):
            _assert_is(ctype, decl, f"{name} parameter {i}")
        if ret == "void":
            assert fn.restype is None, name
        else:
            _assert_is(fn.restype, ret, f"{name} returns")


def _mirrors():
    """(C struct, Python mirror) of every ctypes Structure and numpy dtype of the package"""
    import svtav1_hip as s
    from svtav1_hip import sharded as sh
    return [("svthip_fullpel_desc", s.FullpelDesc), ("svthip_pa_picture", s.PaPictureDesc), ("svthip_me_params", s.MeParams),
            ("svthip_sb_origin", s.SbOrigin), ("svthip_me_cu_result", s.MeCuResult), ("svthip_me_cu_result", s.ME_CU_RESULT_DTYPE),
            ("svthip_quant_desc", s.QUANT_DESC_DTYPE), ("svthip_txfm_desc", s.TXFM_DESC_DTYPE), ("svthip_itxfm_desc", s.ITXFM_DESC_DTYPE),
            ("svthip_tu_desc", s.TU_DESC_DTYPE), ("svthip_convolve_desc", s.CONVOLVE_DESC_DTYPE),
            ("svthip_convolve_compound_desc", s.CONVOLVE_COMPOUND_DESC_DTYPE), ("svthip_inter_planes", s.InterPlanes),
            ("svthip_inter_pu_desc", s.INTER_PU_DESC_DTYPE), ("svthip_warp_pu_desc", s.WARP_PU_DESC_DTYPE), ("svthip_intra_desc", s.INTRA_DESC_DTYPE),
            ("svthip_cfl_desc", s.CFL_DESC_DTYPE), ("svthip_cfl_decision_job", s.CFL_DECISION_JOB_DTYPE), ("svthip_cfl_decision", s.CFL_DECISION_DTYPE),
            ("svthip_lf_mi", s.LF_MI_DTYPE), ("svthip_lf_picture", s.LfPicture), ("svthip_cdef_picture", s.CdefPicture),
            ("svthip_cdef_result", s.CDEF_RESULT_DTYPE), ("svthip_lr_picture", s.LrPicture), ("svthip_wiener_walk_state", s.WIENER_WALK_STATE_DTYPE),
            ("svthip_sgrproj_detail", s.SGRPROJ_DETAIL_DTYPE), ("svthip_tu_result", s.TuResult), ("svthip_lv_map_coeff_cost", s.LV_MAP_COEFF_COST_DTYPE),
            ("svthip_coeff_rate_tables", s.COEFF_RATE_TABLES_DTYPE), ("svthip_coeff_rate_desc", s.COEFF_RATE_DESC_DTYPE),
            ("svthip_tx_search_tu", s.TxSearchTu), ("svthip_tx_search_result", s.TxSearchResult), ("svthip_me_cu_result_ref", s.ME_CU_RESULT_REF_DTYPE),
            ("svthip_host_picture", s.HostPicture), ("svthip_ois_params", s.OisParams), ("svthip_recon_picture", sh.ReconPicture),
            ("svthip_xfer", sh.Xfer)]


RENAMED_FIELDS = {"lambda_": "lambda"}   # Python field -> C field
# Python constant -> the #define it mirrors
CONSTANTS = {"NUM_SQ_PU": "SVTHIP_NUM_SQ_PU", "MAX_SAD_VALUE": "SVTHIP_MAX_SAD_VALUE", "OPT_SADLOOP_GENERIC": "SVTHIP_OPT_SADLOOP_GENERIC",
             "OPT_CONVOLVE_VALU": "SVTHIP_OPT_CONVOLVE_VALU", "OPT_TQ_MAX_WORKGROUPS": "SVTHIP_OPT_TQ_MAX_WORKGROUPS",
             "HME_MAX_JOBS": "SVTHIP_HME_MAX_JOBS", "FRACTIONAL_SUB_SAD_SEARCH": "SVTHIP_FRACTIONAL_SUB_SAD_SEARCH",
             "FRACTIONAL_FULL_SAD_SEARCH": "SVTHIP_FRACTIONAL_FULL_SAD_SEARCH", "FRACTIONAL_SSD_SEARCH": "SVTHIP_FRACTIONAL_SSD_SEARCH",
             "CDEF_PICK_MAX_FB": "SVTHIP_CDEF_PICK_MAX_FB", "RESTORE_NONE": "SVTHIP_RESTORE_NONE", "RESTORE_WIENER": "SVTHIP_RESTORE_WIENER",
             "RESTORE_SGRPROJ": "SVTHIP_RESTORE_SGRPROJ", "TU_RECON_SCRATCH": "SVTHIP_TU_RECON_SCRATCH"}


def test_no_mirror_is_missing_from_the_table():
    import svtav1_hip
    from svtav1_hip import sharded
    mirrors = _mirrors()
    assert len(mirrors) == 37
    for module in (svtav1_hip, sharded):
        for name, v in vars(module).items():
            if name.endswith("_DTYPE") or (isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure):
                assert any(v is m for _, m in mirrors), f"{module.__name__}.{name} mirrors a C struct and is not in the table of this test"


def test_layouts_and_constants_equal_the_headers():
    import svtav1_hip
    lines = ["#include <stddef.h>", '#include "svtav1_hip.h"']
    for i, (cname, py) in enumerate(_mirrors()):
        if isinstance(py, np.dtype):
            size, fields = py.itemsize, [(k, py.fields[k][1]) for k in py.names]
        else:
            size, fields = C.sizeof(py), [(k, getattr(py, k).offset) for k, _ in py._fields_]
        lines.append(f"typedef char m{i}_size[sizeof({cname}) == {size} ? 1 : -1];")
        lines += [f"typedef char m{i}_{k}[offsetof({cname}, {RENAMED_FIELDS.get(k, k)}) == {o} ? 1 : -1];" for k, o in fields]
    for py_name, define in CONSTANTS.items():
        value = getattr(svtav1_hip, py_name)
        assert isinstance(value, int)
        lines.append(f"typedef char c_{py_name}[({define}) == {value} ? 1 : -1];")
    lines.append("int main(void) { return 0; }")
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "binding_layout.c")
        with open(c, "w") as f:
            f.write("\n".join(lines) + "\n")
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", c],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _ints(v):
    return isinstance(v, int) or (isinstance(v, (tuple, list)) and all(_ints(x) for x in v))


def _describe(v):
    """what tests/golden/binding_surface.json records of one public name"""
    if isinstance(v, type) and issubclass(v, C.Structure):
        return {"fields": [[f[0], f[1].__name__] for f in v._fields_]}
    if isinstance(v, np.dtype):
        return {"descr": repr(v.descr)}
    if _ints(v):
        return {"value": repr(v)}
    if callable(v):
        try:
            return {"signature": str(inspect.signature(v))}
        except (ValueError, TypeError):
            pass
    return {"kind": type(v).__name__}


def test_public_surface_is_the_recorded_one():
    """every name recorded at the commit before this test existed is still there with the same signature / value / layout; new names may come"""
    import svtav1_hip
    from svtav1_hip import sharded
    scopes = {"svtav1_hip": svtav1_hip, "svtav1_hip.sharded": sharded, "svtav1_hip.Context": svtav1_hip.Context,
              "svtav1_hip.TuBatcher": svtav1_hip.TuBatcher, "svtav1_hip.sharded.Comm": sharded.Comm,
              "svtav1_hip.sharded.ShardedMotionEstimation": sharded.ShardedMotionEstimation, "svtav1_hip.sharded.ReconExchange": sharded.ReconExchange}
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "binding_surface.json")))
    assert set(recorded) == set(scopes) and sum(len(v) for v in recorded.values()) >= 186
    for scope, names in recorded.items():
        for name, want in names.items():
            assert hasattr(scopes[scope], name), f"{scope}.{name} is gone"
            v = getattr(scopes[scope], name)
            assert not isinstance(v, types.ModuleType) and _describe(v) == want, (f"{scope}.{name}", _describe(v), want)
