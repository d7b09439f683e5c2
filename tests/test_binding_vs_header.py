"""The Python package against include/svtav1_hip.h (no GPU needed): the signatures the package sets on the library are the header's, the
layouts and constants the package reads from the header (_abi) are the compiler's for every struct and #define, every layout the package
offers is one of those, and the package's public surface is the one recorded in tests/golden/binding_surface.json before the signatures were read from the header."""
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


# mirrors the recorded surface keeps in a form the header does not give: Python name -> C struct (the reason stands beside each in the package)
HAND_WRITTEN = {"ME_CU_RESULT_REF_DTYPE": "svthip_me_cu_result_ref", "COEFF_RATE_TABLES_DTYPE": "svthip_coeff_rate_tables"}
RENAMES = ({}, {"lambda_": "lambda"})   # the spellings of the C field `lambda` the package uses: dtype(x) and dtype(x, lambda_="lambda")


def _header_struct_names():
    """the name of every `typedef struct {...} name;`, read here a second time, independently of the package"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names, open_braces = [], []
    for m in re.finditer(r"typedef\s+struct\b[^;{]*\{|[{}]", text):
        if m.group(0) != "}":
            open_braces.append(m.group(0) != "{")
        elif open_braces.pop():   # the brace that closes a typedef struct: its name follows
            names.append(re.match(r"\s*(\w+)\s*;", text[m.end():]).group(1))
    return names


def _offsets(dt, prefix=""):
    """(C member designator, offset) of every field of a dtype; the fields of a nested struct through its element [0] or the member itself"""
    for k in dt.names:
        sub, at = dt.fields[k][0], dt.fields[k][1]
        yield prefix + k, at
        if sub.base.names:
            first = prefix + k + "[0]" * len(sub.shape) + "."
            yield from ((name, at + o) for name, o in _offsets(sub.base, first))


def _compile(lines, what):
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "binding_layout.c")
        with open(c, "w") as f:
            f.write("\n".join(["#include <stddef.h>", '#include "svtav1_hip.h"'] + [line for _, line in lines] + ["int main(void) { return 0; }"]) + "\n")
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.dirname(HEADER), "-fsyntax-only", c],
                           capture_output=True, text=True)
        # gcc names the failed typedef by its line: 3 is the first of `lines`
        failed = sorted({lines[int(n) - 3][0] for n in re.findall(r"binding_layout\.c:(\d+):\d+: error", r.stderr) if 3 <= int(n) < 3 + len(lines)})
        assert r.returncode == 0, f"{what} differ from the header: {failed}\n{r.stderr[:2000]}"


def test_structs_are_exactly_the_headers():
    from svtav1_hip import _abi
    names = _header_struct_names()
    assert len(names) == len(set(names)) >= 53
    assert set(_abi.structs()) == set(names)


def test_layouts_and_constants_equal_the_headers():
    """sizeof and every offsetof of every struct of the header against what _abi derives, as numpy dtype and as ctypes Structure; the same for
    the hand-written mirrors; every #define with a value against define()"""
    import svtav1_hip
    from svtav1_hip import _abi
    lines = []
    for cname in _abi.structs():
        dt, st = _abi.dtype(cname), _abi.structure(cname)
        assert dt.itemsize == C.sizeof(st) and dt.names == tuple(k for k, _ in st._fields_), cname
        lines.append((cname, f"typedef char s{len(lines)}[sizeof({cname}) == {dt.itemsize} ? 1 : -1];"))
        for k, o in _offsets(dt):
            lines.append((f"{cname}.{k}", f"typedef char s{len(lines)}[offsetof({cname}, {k}) == {o} ? 1 : -1];"))
        for k, _ in st._fields_:
            lines.append((f"{cname}.{k}", f"typedef char s{len(lines)}[offsetof({cname}, {k}) == {getattr(st, k).offset} ? 1 : -1];"))
            lines.append((f"{cname}.{k}", f"typedef char s{len(lines)}[sizeof((({cname} *)0)->{k}) == {getattr(st, k).size} ? 1 : -1];"))
    for py_name, cname in HAND_WRITTEN.items():
        dt = getattr(svtav1_hip, py_name)
        lines.append((py_name, f"typedef char s{len(lines)}[sizeof({cname}) == {dt.itemsize} ? 1 : -1];"))
        for k, o in _offsets(dt):
            lines.append((f"{py_name}.{k}", f"typedef char s{len(lines)}[offsetof({cname}, {k}) == {o} ? 1 : -1];"))
    defines = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SVTHIP_\w+)[ \t]+\S", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S), flags=re.M)
    assert len(defines) >= 44
    mirrored = 0
    for name in defines:
        lines.append((name, f"typedef char s{len(lines)}[({name}) == {_abi.define(name)} ? 1 : -1];"))
        if hasattr(svtav1_hip, name[len("SVTHIP_"):]):   # the package's constant of the same name is that value
            value = getattr(svtav1_hip, name[len("SVTHIP_"):])
            assert isinstance(value, int) and value == _abi.define(name), name
            mirrored += 1
    assert mirrored >= 30
    _compile(lines, "layouts or constants")


def test_every_layout_of_the_package_is_derived_from_the_header():
    """every public numpy dtype, function returning one and ctypes Structure of the package is the object _abi derives for a header struct"""
    import svtav1_hip
    from svtav1_hip import _abi, sharded
    derived = [f(cname, **r) for cname in _abi.structs() for r in RENAMES for f in (_abi.dtype, _abi.structure)
               if set(r.values()) <= {k for k, _, _ in _abi.structs()[cname]}]
    found = 0
    for module in (svtav1_hip, sharded):
        for name, v in vars(module).items():
            if name.startswith("_"):
                continue
            if inspect.isfunction(v) and inspect.signature(v).return_annotation in ("np.dtype", np.dtype):
                v = v()
            if isinstance(v, np.dtype) or (isinstance(v, type) and issubclass(v, C.Structure)):
                found += 1
                assert name in HAND_WRITTEN or any(v is d for d in derived), f"{module.__name__}.{name} states a layout of its own"
    assert found >= 50 and all(hasattr(svtav1_hip, k) for k in HAND_WRITTEN)
    from svtav1_hip import _analysis
    assert _analysis._Planes is _abi.structure("svthip_planes")


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
