"""CPU: the partition entries in the library and the header -- the symbols, the C99 header, the sizes of the five 16-byte records as the
md_partition_*_dtype() functions of the package give them, and every refusal the entries make on the host: those are checked before the
context is entered, so they need no device (a null context is what a call with good arguments is refused for here)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import abi_util
import svtav1_hip
from svtav1_hip import _abi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LAYOUTS = (("svthip_md_partition_block", svtav1_hip.md_partition_block_dtype), ("svthip_md_partition_sb", svtav1_hip.md_partition_sb_dtype),
           ("svthip_md_partition_leaf", svtav1_hip.md_partition_leaf_dtype), ("svthip_md_partition_result", svtav1_hip.md_partition_result_dtype),
           ("svthip_md_partition_final", svtav1_hip.md_partition_final_dtype))


def test_symbols_are_exported_and_bound():
    lib = svtav1_hip.lib()
    for name, n_args in (("svthip_md_partition_geometry", 3), ("svthip_md_partition_batch_dev", 14), ("svthip_md_partition_compose_dev", 14),
                         ("svthip_md_partition_picture_dev", 20)):
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args, name
    for method in ("md_partition_batch_dev", "md_partition_compose_dev", "md_partition_picture_dev"):
        assert callable(getattr(svtav1_hip.Context, method))


def test_header_is_c99_and_layouts_match(tmp_path):
    for cname, dtype in LAYOUTS:
        dt = dtype()
        assert dt is _abi.dtype(cname)
        abi_util.assert_sizes((dt, 16), (_abi.structure(cname), 16))
        assert sum(dt.fields[k][0].itemsize for k in dt.names) == 16   # no padding the dtype does not see
    names = ("NONE", "SPLIT_FLAG", "TESTED", "MDC_SPLIT_FLAG", "BLOCKS_64", "BLOCKS_128", "MAX_FINAL_64", "MAX_FINAL_128")
    assert [getattr(svtav1_hip, "MD_PART_" + k) for k in names] == [_abi.define("SVTHIP_MD_PART_" + k) for k in names] == \
        [0xFFFFFFFF, 1, 2, 4, 1101, 4421, 256, 1024]
    c = tmp_path / "md_part_header.c"
    c.write_text('#include <stddef.h>\n#include "svtav1_hip.h"\n'
                 + "".join(f"typedef char size_of_{n[7:]}[sizeof({n}) == 16 ? 1 : -1];\n" for n, _ in LAYOUTS)
                 + "typedef char cost_at[offsetof(svthip_md_partition_result, cost) == 0 && offsetof(svthip_md_partition_result, leaf) == 8 ? 1 : -1];\n"
                 "typedef char leaf_at[offsetof(svthip_md_partition_leaf, mds_idx) == 4 && offsetof(svthip_md_partition_leaf, pool_x) == 8 ? 1 : -1];\n"
                 "int main(void) { svthip_md_partition_block b; return svthip_md_partition_geometry(64, &b, 1) != SVTHIP_MD_PART_BLOCKS_64 || "
                 "svthip_md_partition_batch_dev(0, 0, 0, 0, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0) == 0 || "
                 "svthip_md_partition_compose_dev(0, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0, 0, 0, 0) == 0 || "
                 "svthip_md_partition_picture_dev(0, 0, 0, 0, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == 0; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:2000]


def test_geometry_refusals_and_partial_tables():
    lib = svtav1_hip.lib()
    assert [int(lib.svthip_md_partition_geometry(z, None, 0)) for z in (64, 128, 0, 32, 256, 65)] == [1101, 4421, 0, 0, 0, 0]
    with pytest.raises(ValueError):
        svtav1_hip.md_partition_geometry(32)
    part = np.full(10, 0xEE, np.uint8).view(np.uint8).repeat(16).view(svtav1_hip.md_partition_block_dtype())
    assert int(lib.svthip_md_partition_geometry(64, part.ctypes.data, 4)) == 1101
    assert np.array_equal(part[:4], svtav1_hip.md_partition_geometry(64)[:4]) and (part[4:].view(np.uint8) == 0xEE).all()   # `max` records and no more


class _NoContext:   # the partition methods read nothing of a Context but its handle
    _h = None


def _refused(method, *args):
    with pytest.raises(svtav1_hip.SvtHipError) as e:
        getattr(svtav1_hip.Context, method)(_NoContext(), *args)
    return str(e.value)


def test_every_host_refusal():
    buf = np.zeros(4096, np.uint8)
    a = (buf.ctypes.data + 15) & ~15   # a 16-byte aligned address the entries never read: every call here is refused before a launch
    fac = np.zeros((20, 11), np.int32)
    planes = svtav1_hip.InterPlanes(a, a, a, 64, 32)
    batch = lambda **kw: _refused("md_partition_batch_dev", *[kw.get(k, v) for k, v in (  # noqa: E731
        ("d_sb", a), ("n_sb", 1), ("d_leaf", a), ("n_leaf", 1), ("d_decision", a), ("n_decision", 1), ("sb_size", 64), ("intra", 0), ("fac", fac),
        ("d_result", a), ("d_final", a), ("d_count", a))])
    compose = lambda **kw: _refused("md_partition_compose_dev", *[kw.get(k, v) for k, v in (  # noqa: E731
        ("n_sb", 1), ("d_leaf", a), ("n_leaf", 1), ("sb_size", 64), ("d_final", a), ("d_count", a), ("pool", planes), ("pool_w", 64), ("pool_h", 64),
        ("dst", planes), ("w", 64), ("h", 64))])
    picture = lambda **kw: _refused("md_partition_picture_dev", *[kw.get(k, v) for k, v in (  # noqa: E731
        ("d_sb", a), ("n_sb", 1), ("d_leaf", a), ("n_leaf", 1), ("d_decision", a), ("n_decision", 1), ("sb_size", 64), ("intra", 0), ("fac", fac),
        ("d_result", a), ("d_final", a), ("d_count", a), ("pool", planes), ("pool_w", 64), ("pool_h", 64), ("dst", planes), ("w", 64), ("h", 64))])
    # good arguments get as far as the context
    assert all("null context" in f() for f in (batch, compose, picture))
    assert all("null context" in f(n_sb=0) for f in (batch, compose, picture))   # n_sb == 0 is OK only with a context
    for f in (batch, compose, picture):
        for z in (0, 32, 96, 256):
            assert "sb_size must be 64 or 128" in f(sb_size=z)
        assert "sb_size" in f(sb_size=32, n_sb=0)   # the size is refused whatever n_sb
        for k in ("d_leaf", "d_final", "d_count"):
            assert "null pointer" in f(**{k: None}), k
        for k in ("d_leaf", "d_final"):
            assert "16-byte aligned" in f(**{k: a + 8}), k
        assert "16-byte aligned" in f(d_count=a + 2)
        assert "null context" in f(d_count=a + 4)
    for f in (batch, picture):
        for k in ("d_sb", "d_decision", "fac", "d_result"):
            assert "null pointer" in f(**{k: None}), k
        for k in ("d_sb", "d_decision", "d_result"):
            assert "16-byte aligned" in f(**{k: a + 4}), k
    for f in (compose, picture):
        for k in ("pool", "dst"):
            assert "null pointer" in f(**{k: None}), k
            for plane in range(3):
                p = svtav1_hip.InterPlanes(*[None if i == plane else a for i in range(3)], 64, 32)
                assert "null pointer" in f(**{k: p}), (k, plane)
        for k in ("pool_w", "pool_h", "w", "h"):
            assert "must not be 0" in f(**{k: 0}), k
        assert "stride" in f(w=65) and "stride" in f(pool_w=66)
        assert "stride" in f(dst=svtav1_hip.InterPlanes(a, a, a, 64, 31)) and "stride" in f(pool=svtav1_hip.InterPlanes(a, a, a, 63, 32))
    assert C.sizeof(_abi.structure("svthip_md_partition_final")) == 16
