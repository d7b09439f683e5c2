"""Writes tests/golden/film_grain.npz from the reference's own film-grain synthesis (tests/golden/ref_film_grain_driver.c, linked by the
recipe of oracle/ref_driver.py against the reference objects of the oracle build, oracle/_ref/obj_all, with grainSynthesis.o left out: the
driver includes that source to reach its static template functions).  Run in the build container only, where the reference exists: the
fixture is data.

    python tests/golden/make_golden_film_grain.py

Cases: film_grain_util.all_cases() -- every size of SIZES x every parameter set x 8 and 10 bits, and 1920x1080 once.  Sources are
film_grain_util.source_planes and are not stored.  Contents: see film_grain_util.fixture.  Whole pictures go through
av1_add_film_grain_run on dense planes; the AV1_WRAPPER cases also through av1_add_film_grain with bordered EbPictureBufferDesc_t of
different origins and strides, and both are asserted to agree.  The restatement (tests/film_grain_util.py) is asserted equal to the
reference for every case and every table while the fixture is written.

Parameter sets with num_y_points == 0 (film_grain_util.REFERENCE_UNSAFE) are NEVER given to the reference: its dealloc_arrays then frees one
pointer more than init_arrays allocated.  They have no entry here and are checked against the restatement alone."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import film_grain_util as fu  # noqa: E402
from make_golden_cdef import save  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402


def build_driver(out_dir):
    """ref_film_grain_driver.c by the recipe of oracle/ref_driver.py, with its signatures"""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_film_grain_driver.c"), out_dir, leave_out=("grainSynthesis.o",),
                                include=(os.path.join(ref_driver.REF_ROOT, "Source", "Lib", "Codec"),))
    V, I = C.c_void_p, C.c_int
    L.drv_fg_params_offsets.argtypes = [V]
    L.drv_fg_tables.argtypes = [V] * 5
    L.drv_fg_run.argtypes = [V] * 4 + [I] * 5
    L.drv_fg_add.argtypes = [V, I, I, I] + [V] * 6
    L.drv_fg_time.restype = C.c_double
    L.drv_fg_time.argtypes = [V, I, I, I, I]
    return L


def _params(p, bit_depth):
    assert p["num_y_points"] > 0, "the reference must never be run with num_y_points == 0"
    q = dict(p)
    q["bit_depth"] = bit_depth
    return C.create_string_buffer(fu.pack_params(q), fu.PARAMS_BYTES)


def reference_tables(L, p, bit_depth):
    """the table block (int16, the header's layout) from the reference's own template and scaling functions"""
    parts = [np.zeros(n, np.int32) for _, n in fu.TABLE_PARTS]
    assert L.drv_fg_tables(_params(p, bit_depth), *[a.ctypes.data for a in parts]) == 0
    block = np.concatenate(parts)
    assert np.abs(block).max() < 1 << 15
    return block.astype(np.int16)


def reference_run(L, p, bit_depth, planes, wrapper=False):
    """the three planes after av1_add_film_grain_run (dense planes, in place on copies) or, wrapper, after av1_add_film_grain"""
    h, w = planes[0].shape
    if wrapper:
        src = [np.ascontiguousarray(a) for a in planes]
        out = [np.zeros_like(a) for a in src]
        rc = L.drv_fg_add(_params(p, bit_depth), w, h, bit_depth, *[a.ctypes.data for a in src], *[a.ctypes.data for a in out])
        assert rc == 0, ("av1_add_film_grain touched a border sample or its source" if rc == -2 else rc)
        return out
    out = [np.ascontiguousarray(a).copy() for a in planes]
    assert L.drv_fg_run(_params(p, bit_depth), *[a.ctypes.data for a in out], w, h, w, w // 2, bit_depth) == 0
    return out


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    out = {"sizes": np.array(fu.SIZES, np.int32), "big": np.array(fu.BIG, np.int32),
           "params": np.stack([np.frombuffer(fu.pack_params(p), np.uint8) for p in fu.PARAM_SETS])}
    digests = np.zeros((len(fu.SIZES) + 1, len(fu.PARAM_SETS), 2), np.uint64)
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        assert L.drv_fg_params_size() == fu.PARAMS_BYTES
        for s, p in enumerate(fu.PARAM_SETS):
            for bd in fu.BIT_DEPTHS:
                if s in fu.REFERENCE_UNSAFE:
                    continue
                ref = reference_tables(L, p, bd)
                mine = fu.tables_block(fu.tables_of(s, bd))
                assert np.array_equal(mine, ref), ("the restatement's tables differ from the reference", s, bd, np.flatnonzero(mine != ref)[:8])
                out[f"tables_s{s}_b{bd}"] = ref
        for s, bd, z in fu.all_cases():
            if s in fu.REFERENCE_UNSAFE:
                continue
            w, h = fu.size_of(z)
            p = fu.PARAM_SETS[s]
            planes = fu.source_planes(w, h, bd, s)
            ref = reference_run(L, p, bd, planes)
            mine = fu.add_film_grain(p, bd, *planes, t=fu.tables_of(s, bd))
            for k, a, b in zip("y cb cr".split(), mine, ref):
                assert a.dtype == b.dtype and np.array_equal(a, b), ("the restatement differs from the reference", (w, h), s, bd, k, np.argwhere(a != b)[:8])
            digests[z, s, fu.BIT_DEPTHS.index(bd)] = fu.digest(ref)
            wrapped = (z, s, bd) in fu.AV1_WRAPPER
            if wrapped:
                for a, b in zip(reference_run(L, p, bd, planes, wrapper=True), ref):
                    assert np.array_equal(a, b), ("av1_add_film_grain and av1_add_film_grain_run disagree", (w, h), s, bd)
            if wrapped or (z in fu.KEPT and (s, bd) in fu.KEPT[z]):
                for k, a in zip("y cb cr".split(), ref):
                    out[f"out_z{z}_s{s}_b{bd}_{k}"] = a
            print("case", (w, h), "set", s, "bits", bd, "changed", [int((a != b).sum()) for a, b in zip(ref, planes)], "wrapper" if wrapped else "")
    out["digest"] = digests
    cov = fu.coverage([(fu.PARAM_SETS[s], bd, *fu.size_of(z)) for s, bd, z in fu.all_cases() if z < len(fu.SIZES)])
    print("coverage", cov)
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    out["coverage_keys"] = np.array(fu.COVERAGE_KEYS, dtype="U40")
    save(fu.FIXTURE, out)
    print(f"wrote {fu.FIXTURE}: {os.path.getsize(fu.FIXTURE)} bytes")
    assert os.path.getsize(fu.FIXTURE) <= 450_000


if __name__ == "__main__":
    main()
