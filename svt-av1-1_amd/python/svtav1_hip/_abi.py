"""The ctypes signature of every svthip_* entry, read from include/svtav1_hip.h: the header is the one place a signature is written.

A pointer or array parameter becomes c_void_p (it takes byref(x), ctypes arrays, integers and None, not a bare Structure), a scalar the
ctypes type of the same name.  A type the table does not know raises and names the function: nothing is guessed."""
import ctypes as C
import os
import re

HEADER_PATH = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "..", "include", "svtav1_hip.h"))
SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint16_t": C.c_uint16, "size_t": C.c_size_t}
_PROTOTYPE = re.compile(r"(?<=[;{}])\s*([\w\s*]+?)\b(svthip_\w+)\s*\(([^;{}()]*)\)\s*;")


def _scalar(decl: str, name: str):
    words = [w for w in decl.split() if w != "const"]
    if len(words) != 1 or words[0] not in SCALARS:
        raise TypeError(f"{name}: no ctypes type for `{decl.strip()}` in {HEADER_PATH}")
    return SCALARS[words[0]]


def prototypes() -> dict:
    """{name: (return type, [parameter types])} of every prototype of the header"""
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} is missing: the binding reads its signatures from it")
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER_PATH).read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        if "*" in ret:
            ret_t = C.c_char_p if ret.split() == ["const", "char", "*"] else C.c_void_p
        else:
            ret_t = None if ret.split() == ["void"] else _scalar(ret, name)
        arg_ts = []
        for p in ([] if params.split() == ["void"] else params.split(",")):
            # a scalar parameter is `type name`: everything before its last word is the type
            arg_ts.append(C.c_void_p if "*" in p or "[" in p else _scalar(" ".join(p.split()[:-1]), name))
        out[name] = (ret_t, arg_ts)
    missed = set(re.findall(r"\b(svthip_\w+)\s*\(", text)) - set(out)
    if missed:
        raise TypeError(f"{sorted(missed)}: declared in {HEADER_PATH} in a form the binding does not read")
    return out


def bind(library: C.CDLL) -> None:
    for name, (ret_t, arg_ts) in prototypes().items():
        fn = getattr(library, name)
        fn.restype, fn.argtypes = ret_t, arg_ts
