"""Everything the binding knows of the C ABI, read from include/svtav1_hip.h: the header is the one place a signature, a struct layout or a
constant is written.

prototypes() gives the ctypes signature of every svthip_* entry: a pointer or array parameter becomes c_void_p (it takes byref(x), ctypes
arrays, integers and None, not a bare Structure), a scalar the ctypes type of the same name.  structs() gives the fields of every
`typedef struct`, dtype() / structure() the numpy and ctypes mirror of one (both pad the way C does), define() the integer value of a
#define.  A form the reader does not know raises and names the function, struct or constant: nothing is guessed."""
import ctypes as C
import functools
import os
import re

import numpy as np

HEADER_PATH = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "..", "include", "svtav1_hip.h"))
SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint16_t": C.c_uint16, "size_t": C.c_size_t}
FIELD_TYPES = {"int8_t": C.c_int8, "uint8_t": C.c_uint8, "int16_t": C.c_int16, "uint16_t": C.c_uint16, "int32_t": C.c_int32,
               "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}
POINTER = "*"   # the type structs() gives a pointer field, whatever it points to
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


@functools.lru_cache(maxsize=None)
def _header():
    """(header without comments, {macro: replacement text})"""
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} is missing: the binding reads its layouts and constants from it")
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER_PATH).read(), flags=re.S)
    return text, dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M))


@functools.lru_cache(maxsize=None)
def define(name: str) -> int:
    """the value of an integer #define: literals (a `u` suffix allowed), other defines, + - * << | and an (int32_t) cast"""
    macros = _header()[1]
    if name not in macros:
        raise KeyError(f"{name}: no #define with a value in {HEADER_PATH}")
    expr = re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uU]?\b", r"\1", macros[name])
    expr = re.sub(r"\b[A-Za-z_]\w*\b", lambda m: m.group(0) if m.group(0) == "int32_t" else str(define(m.group(0))), expr)
    expr = re.sub(r"\(\s*int32_t\s*\)\s*(\w+)", r"((\1 + 2**31) % 2**32 - 2**31)", expr)
    if not re.fullmatch(r"[0-9a-fA-FxX\s()+\-*%<|]+", expr):
        raise TypeError(f"{name}: `{macros[name]}` in {HEADER_PATH} is not an integer expression the binding reads")
    return int(eval(expr, {"__builtins__": {}}))


def _fields(body: str, struct: str, known) -> tuple:
    """the `type declarator[, declarator];` statements of a struct body; an anonymous inner struct has its own field list for a type"""
    out = []
    while body.strip():
        inner = re.match(r"\s*struct\s*\{([^{}]*)\}([^;]*);", body)
        m = inner or re.match(r"\s*((?:const\s+)?)(\w+)\b([^;{}]*);", body)
        if not m:
            raise TypeError(f"{struct}: `{' '.join(body.split())[:60]}` in {HEADER_PATH} is not a field declaration the binding reads")
        body = body[m.end():]
        base, declarators = (_fields(inner.group(1), struct, known), inner.group(2)) if inner else (m.group(2), m.group(3))
        for d in declarators.split(","):
            dm = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*((?:\[\s*\w+\s*\]\s*)*)", d)
            if not dm or (dm.group(1) and inner) or not (dm.group(1) or inner or base in FIELD_TYPES or base in known):
                raise TypeError(f"{struct}: no layout for `{' '.join((m.group(0)).split())}` in {HEADER_PATH}")
            dims = tuple(int(n) if n.isdigit() else define(n) for n in re.findall(r"\[\s*(\w+)\s*\]", dm.group(3)))
            out.append((dm.group(2), POINTER if dm.group(1) else base, dims))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def structs() -> dict:
    """{C name: [(field, type, dims), ...]} of every `typedef struct {...} svthip_x;`: type is a name of FIELD_TYPES, POINTER, the name of
    an earlier struct, or the fields of an anonymous inner struct as a tuple; dims is () for a scalar"""
    text = re.sub(r"^\s*#.*$", " ", _header()[0], flags=re.M)
    out = {}
    for m in re.finditer(r"\btypedef\s+struct\s*\w*\s*\{((?:[^{}]|\{[^{}]*\})*)\}\s*(\w+)\s*;", text):
        out[m.group(2)] = list(_fields(m.group(1), m.group(2), out))
    if len(out) != len(re.findall(r"\btypedef\s+struct\s*\w*\s*\{", text)):
        raise TypeError(f"a `typedef struct` of {HEADER_PATH} is in a form the binding does not read")
    return out


def _renamed(struct, renamed):
    """the fields of a header struct (its name) or an inner struct (its fields), the C names of `renamed` replaced"""
    fields = struct if isinstance(struct, tuple) else structs()[struct]
    c_names = [f[0] for f in fields]
    if not set(renamed.values()) <= set(c_names):
        raise KeyError(f"no field {sorted(set(renamed.values()) - set(c_names))} to rename")
    back = {c: py for py, c in renamed.items()}
    return [(back.get(name, name), t, dims) for name, t, dims in fields]


@functools.lru_cache(maxsize=None)
def _dtype(c_name, renamed):
    kind = lambda t: np.uintp if t == POINTER else FIELD_TYPES[t] if t in FIELD_TYPES else _dtype(t, ())
    return np.dtype([(name, kind(t)) + ((dims,) if dims else ()) for name, t, dims in _renamed(c_name, dict(renamed))], align=True)


@functools.lru_cache(maxsize=None)
def _structure(c_name, renamed):
    members = []
    for name, t, dims in _renamed(c_name, dict(renamed)):
        ct = C.c_void_p if t == POINTER else FIELD_TYPES[t] if t in FIELD_TYPES else _structure(t, ())
        for n in reversed(dims):
            ct = ct * n
        members.append((name, ct))
    return type(c_name if isinstance(c_name, str) else "inner", (C.Structure,), {"_fields_": members})


def dtype(c_name: str, **renamed) -> np.dtype:
    """the numpy mirror of a header struct (one object per layout); dtype(x, lambda_="lambda") spells the C field `lambda` lambda_"""
    return _dtype(c_name, tuple(sorted(renamed.items())))


def structure(c_name: str, **renamed) -> type:
    """the ctypes.Structure mirror of a header struct (one class per layout); fields are renamed as for dtype()"""
    return _structure(c_name, tuple(sorted(renamed.items())))
