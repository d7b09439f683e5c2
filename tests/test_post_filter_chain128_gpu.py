"""GPU: the front of the post-reconstruction chain on pictures coded with 128-wide blocks, against tests/golden/post_filter_chain128.npz
(the reference's own stages run as a chain on two 328 x 200 pictures; tests/post_filter_chain128_util.py).

  av1_pick_filter_level_dev -> av1_loop_filter_frame_dev (the levels stay in d_levels) -> av1_cdef_search128_dev on the same d_mi ->
  av1_cdef_frame_dev

The grid the deblocking entries read is the grid the CDEF search reads: one upload.  Between the first call and the last there is no host
synchronisation; after one wait levels, tables, strengths and planes are compared in chain order and the first stage that differs is
named.  This is where the deblocking kernels meet BLOCK_128X128, BLOCK_128X64 and BLOCK_64X128 with TX_64X64."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import cdef_util as cu  # noqa: E402
import post_filter_chain128_util as pc128  # noqa: E402
import post_filter_chain_util as pc  # noqa: E402
import svtav1_hip  # noqa: E402
from lr_gpu_util import Guarded, _dev, _ready  # noqa: E402
from test_cdef_gpu import SKIP_GUARD, Table  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tuple(pc128.PICTURES))
def test_chain_with_128_wide_blocks(hip_ctx, name):
    torch = pytest.importorskip("torch")
    P = pc128.PICTURES[name]
    bd, w, h, q = P["bd"], pc128.W, pc128.H, P["base_qindex"]
    mi, recon0, source0 = pc128.make_picture(name)
    want = pc128.expected(name, recon0)
    for k, v in pc.input_digests(mi, recon0, source0).items():
        assert np.array_equal(v, want["sha256_" + k]), f"picture {name}: the regenerated {k} is not the fixture's input"
    recon, source = Guarded(torch, recon0, bd), Guarded(torch, source0, bd, extra=2)
    cdef = Guarded(torch, [np.full_like(p, 7) for p in recon0], bd, extra=4)
    d_mi = _dev(torch, mi)
    skip, _ = pc128.grids(mi)
    sk = np.ones((skip.shape[0] + 2, skip.shape[1] + SKIP_GUARD), np.uint8)
    sk[1:-1, 1:1 + skip.shape[1]] = skip
    d_skip = _dev(torch, sk)
    nh, nv = cu.geometry(w, h)
    nfb = nh * nv
    levels, sse_tables, masks = Table(torch, 4, np.int32, -77), Table(torch, 5 * 64, np.uint64, 0x5A5A5A5A5A5A5A5A), Table(torch, 5, np.uint64, 0x5A5A5A5A5A5A5A5A)
    mse, counted = Table(torch, 2 * nfb * 64, np.uint64, 0x5A5A5A5A5A5A5A5A), Table(torch, nfb, np.uint8, 0x5A)
    result, fbs = Table(torch, 21, np.int32, -77), Table(torch, nfb, np.int8, 0x5A)
    work = Table(torch, svtav1_hip.cdef_search128_workspace_bytes(w, h) // 8, np.uint64, 0x3C3C3C3C3C3C3C3C)
    lf = svtav1_hip.make_lf_picture(w, h, recon.ptr, recon.stride, source.ptr, source.stride)
    pic = svtav1_hip.make_cdef_picture(w, h, recon.ptr, recon.stride, d_skip.data_ptr() + sk.shape[1] + 1, sk.shape[1], source.ptr, source.stride, cdef.ptr,
                                       cdef.stride)
    _ready(torch)
    hip_ctx.av1_pick_filter_level_dev(lf, d_mi.data_ptr(), mi.shape[1], P["last_levels"], 0, 0, levels.ptr, sse_tables.ptr, masks.ptr, bit_depth=bd)
    hip_ctx.av1_loop_filter_frame_dev(lf, d_mi.data_ptr(), mi.shape[1], levels.ptr, 0, 0, 3, bit_depth=bd)
    hip_ctx.av1_cdef_search128_dev(pic, q, mse.ptr, counted.ptr, result.ptr, fbs.ptr, d_mi.data_ptr(), mi.shape[1], work.ptr, bit_depth=bd)
    hip_ctx.av1_cdef_frame_dev(pic, result.ptr, fbs.ptr, 0, 3, bit_depth=bd)
    hip_ctx.synchronize()
    (dbk, ok_dbk), (out, ok_out) = recon.planes(), cdef.planes()
    got = {"dbk": dbk, "cdef": out, "levels": levels.get(), "masks": masks.get(), "mse": mse.get(), "counted": counted.get(), "cdef_result": result.get(),
           "fb_strength": fbs.get()}
    diff = pc128.first_difference(got, want)
    assert diff is None, f"picture {name}: the device chain differs from the reference's at {diff}"
    assert ok_dbk and ok_out, "a sample outside the planes was written"
    work.get(), sse_tables.get()
    assert all(np.array_equal(a, b) for a, b in zip(source.planes()[0], source0)), "the source planes were written"
    assert np.array_equal(d_mi.cpu().numpy().view(mi.dtype).reshape(mi.shape), mi), "the mode-info grid was written"
