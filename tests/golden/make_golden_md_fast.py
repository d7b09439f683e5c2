"""Writes tests/golden/md_fast.npz from the reference's own SAD kernels, RDCOST macro and PreModeDecision (tests/golden/ref_md_fast_driver.c,
linked by the recipe of oracle/ref_driver.py against the reference objects of the oracle build, oracle/_ref/obj_all).  Run in the build
container only, where the reference exists: the fixture is data.

    python tests/golden/make_golden_md_fast.py

The inputs are constructed (tests/md_fast_util.py: source_planes, pool_planes, descriptors, pick_cases) and are not stored; their CRCs are,
so that a change of the construction is noticed.  Contents:
  sizes [22][2]              md_fast_util.SIZES
  src_crc [3], pool_crc [22][3]   zlib.crc32 of the source planes and of every size's pool planes
  sads_z{z} [13][3] u32      Y, Cb, Cr SAD of the 13 descriptors of size z from NxMSadKernelSubSampled_funcPtrArray, luma indexed
                             bwidth >> 3 and chroma bwidth >> 4; the ASM_NON_AVX2 and the ASM_AVX2 row are asserted equal
  result_z{z} [13]           RESULT_DTYPE as bytes: the SADs under the descriptor's flags and the cost through the reference's RDCOST
  pick [n_groups][32] u8     PICK_DTYPE of md_fast_util.pick_cases(): the restated walk, then the reference's PreModeDecision
  pick_names                 the names of the cases
While it writes, the restatement is asserted equal to the reference: every SAD, every cost, and best[], the full count and
disable_merge_index of every group.  What the reference cannot be run for -- the buffer walk and the flags of ProductPerformFastLoop, which
drags the prediction tables along -- is the restatement's alone."""
import ctypes as C
import os
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import md_fast_util as mu  # noqa: E402
from make_golden_cdef import save  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

N_DESC = 13   # one descriptor per flag set


def build_driver(out_dir):
    """ref_md_fast_driver.c by the recipe of oracle/ref_driver.py, with its signatures"""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_md_fast_driver.c"), out_dir)
    V = C.c_void_p
    L.drv_md_fast_sad.restype = C.c_int64
    L.drv_md_fast_sad.argtypes = [C.c_int, C.c_int, V, C.c_uint32, V, C.c_uint32, C.c_uint32, C.c_uint32]
    L.drv_md_fast_rdcost.restype = C.c_uint64
    L.drv_md_fast_rdcost.argtypes = [C.c_uint64] * 3
    L.drv_md_fast_pre_mode_decision.argtypes = [C.c_int, V, V, C.c_uint32, C.c_int, V, V, V]
    return L


def crcs(planes):
    return [zlib.crc32(np.ascontiguousarray(p).tobytes()) for p in planes]


def reference_sads(L, src, pred, d, w, h):
    """(Y, Cb, Cr) SADs of one descriptor from the reference's table, both asm rows asserted equal.  The planes are copied so that each
    ends with its last sample: a kernel that read past a block in the last rows would leave the allocation"""
    cw, ch = mu.chroma_size(w, h)
    out = []
    for k in range(3):
        bw, bh, index = (w, h, w >> 3) if k == 0 else (cw, ch, w >> 4)
        x, y, u, v = [int(d[f]) for f in ("src_x", "src_y", "pred_x", "pred_y")]
        if k:
            x, y, u, v = [mu.round_uv(t) for t in (x, y, u, v)]
        s, p = np.ascontiguousarray(src[k]), np.ascontiguousarray(pred[k])
        rows = []
        for asm_type in (0, 1):
            r = L.drv_md_fast_sad(asm_type, index, s.ctypes.data + y * s.shape[1] + x, s.shape[1], p.ctypes.data + v * p.shape[1] + u, p.shape[1], bh, bw)
            assert r >= 0, ("the reference has no SAD kernel at", asm_type, index)
            rows.append(int(r))
        assert rows[0] == rows[1], ("ASM_NON_AVX2 and ASM_AVX2 disagree", (w, h), k, rows)
        out.append(rows[0])
    return tuple(out)


def reference_result(L, d, sads):
    """RESULT_DTYPE scalar of a descriptor: the flags as md_fast_util.finish applies them, the cost through the reference's RDCOST"""
    luma, chroma, cost = mu.finish(d, sads)
    if not int(d["flags"]) & mu.INVALID:
        ref_cost = int(L.drv_md_fast_rdcost(int(d["lambda_"]), min(int(d["rate"]), int(d["merge_rate"])), luma + chroma))
        assert ref_cost == cost, ("the restated RDCOST differs from the reference", d, ref_cost, cost)
    return luma, chroma, cost


def reference_pick(L, g, cost, cand, flags):
    """PICK_DTYPE scalar of a group whose walk left (cost, cand): the reference's PreModeDecision on those buffers"""
    types, total, same = mu.pick_arguments(g, cost, cand, flags)
    c, t = np.array(cost, np.uint64), np.array(types, np.uint8)
    best, full, dmi = np.full(16, 0xFF, np.uint8), C.c_uint32(0), C.c_uint8(0)
    assert L.drv_md_fast_pre_mode_decision(mu.MAX_BUFFERS, c.ctypes.data, t.ctypes.data, total, int(same), best.ctypes.data, C.byref(full), C.byref(dmi)) == 0
    out = np.zeros((), mu.PICK_DTYPE)
    out["best"], out["buffer_cand"] = best[:13], cand
    out["full_count"], out["disable_merge_index"] = full.value, dmi.value
    mine = mu.pre_mode_decision(cost, types, total, same)
    n = total if same else max(1, total - 1)
    assert (list(best[:n]), full.value, dmi.value) == (mine[0][:n], mine[1], mine[2]) and (best[n:13] == 0xFF).all(), \
        ("the restated PreModeDecision differs from the reference", g, list(best), mine)
    return out


def reference_picks(L, result, desc, groups):
    out = np.zeros(len(groups), mu.PICK_DTYPE)
    for i, g in enumerate(groups):
        rows = slice(int(g["first"]), int(g["first"]) + int(g["count"]))
        cost, cand = mu.walk(result["cost"][rows], mu.max_buffers(g))
        out[i] = reference_pick(L, g, cost, cand, desc["flags"][rows])
    return out


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    src = mu.source_planes()
    out = {"sizes": np.array(mu.SIZES, np.int32), "src_crc": np.array(crcs(src), np.uint32), "pool_crc": np.zeros((len(mu.SIZES), 3), np.uint32)}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for z, (w, h) in enumerate(mu.SIZES):
            pool = mu.pool_planes(z, src)
            out["pool_crc"][z] = crcs(pool)
            desc = mu.descriptors(z, N_DESC)
            sads, result = np.zeros((N_DESC, 3), np.uint32), np.zeros(N_DESC, mu.RESULT_DTYPE)
            for i, d in enumerate(desc):
                sads[i] = reference_sads(L, src, pool, d, w, h)
                assert tuple(sads[i]) == mu.candidate_sads(src, pool, d, w, h), ("the restated SAD differs from the reference", (w, h), i)
                result[i] = reference_result(L, d, tuple(int(v) for v in sads[i]))
            assert np.array_equal(result, mu.fast_cost(src, pool, desc, w, h)), (w, h)
            out[f"sads_z{z}"], out[f"result_z{z}"] = sads, result.view(np.uint8).reshape(N_DESC, 16)
            print((w, h), "luma", sads[:6, 0].tolist(), "chroma", (sads[:6, 1] + sads[:6, 2]).tolist())
        cases = mu.pick_cases()
        result, desc, groups = mu.pick_inputs(cases)
        picks = reference_picks(L, result, desc, groups)
        mine, refused = mu.pick(result, desc, groups)
        assert refused == 0 and np.array_equal(picks, mine), "the restated pick differs from the reference"
        for c, p in zip(cases, picks):
            print(c[0], "best", p["best"][:p["full_count"]].tolist(), "full", int(p["full_count"]), "dmi", int(p["disable_merge_index"]))
    out["pick"] = picks.view(np.uint8).reshape(len(groups), 32)
    out["pick_names"] = np.array([c[0] for c in cases], dtype="U64")
    save(mu.FIXTURE, out)
    print(f"wrote {mu.FIXTURE}: {os.path.getsize(mu.FIXTURE) / 1e3:.1f} KB")


if __name__ == "__main__":
    main()
