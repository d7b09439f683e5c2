"""GPU: the CDEF entries for grids with 128-wide blocks bit-exact against the reference's fixture (tests/golden/cdef128.npz): the tables
and counted flags for every case and base_qindex, the pick with its copies on the fixture's tables, the one-call search feeding the existing
frame filter from device memory, the frame filter on the constructed run, case D against the existing entries called on the same picture,
the stage split against the one call, and every new refusal.  Planes, tables, the workspace and the grid sit between guards that must come
back untouched; the grid has exactly height / 4 rows, its guard cells and its row padding name BLOCK_128X128 and its flags are all set, so
a cell read from the wrong place or a skip flag taken from the grid shows.  Every comparison is equality; no case is larger than 328x200."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import cdef128_util as c128  # noqa: E402
import cdef_util as cu  # noqa: E402
import svtav1_hip  # noqa: E402
from lr_gpu_util import _dev  # noqa: E402
from test_cdef128_vs_ref import N_CASES, case_index, fixture_case  # noqa: E402
from test_cdef_gpu import DevCase, Table  # noqa: E402

pytestmark = pytest.mark.gpu
GRID_PAD = 5


class DevCase128(DevCase):
    """DevCase with the mode-info grid (svthip_lf_mi, 4 bytes a cell) and the workspace"""

    def __init__(self, torch, F, sb_type=None):
        super().__init__(torch, F)
        t = F["sb_type"] if sb_type is None else sb_type
        rows, cols = t.shape
        self.mi_stride = cols + GRID_PAD
        g = np.zeros((rows + 2, self.mi_stride, 4), np.uint8)
        g[..., 0], g[..., 1], g[..., 2], g[..., 3] = c128.BLOCK_128X128, 4, 0xFF, 0xA5
        g[1:-1, :cols, 0] = t
        self.grid_host, self.grid = g, _dev(torch, g)
        self.mi = self.grid.data_ptr() + self.mi_stride * 4
        self.work = Table(torch, self.nfb * 3 * 64, np.uint64, 0x3C3C3C3C3C3C3C3C)
        assert self.work.dtype.itemsize * self.nfb * 3 * 64 == svtav1_hip.cdef_search128_workspace_bytes(F["w"], F["h"])

    def inputs_untouched(self):
        self.work.get()
        return super().inputs_untouched() and np.array_equal(self.grid.cpu().numpy().reshape(self.grid_host.shape), self.grid_host)


@pytest.mark.parametrize("c", range(N_CASES))
def test_search_tables_and_counted_flags(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = DevCase128(torch, F)
    for qi, q in enumerate(F["qindex"]):
        hip_ctx.av1_cdef_search_mse128_dev(D.pic, q, D.mse.ptr, D.counted.ptr, D.mi, D.mi_stride, D.work.ptr, bit_depth=D.bd)
        hip_ctx.synchronize()
        mse, counted = D.tables()
        assert np.array_equal(counted, F["counted"]), (c, q, counted, F["counted"])
        assert np.array_equal(mse, F["mse"][qi]), (c, q, np.argwhere(mse != F["mse"][qi])[:8])
    assert D.inputs_untouched()
    assert D.out.planes()[1] and all((p == 7).all() for p in D.out.planes()[0]), "a search entry wrote a picture"


@pytest.mark.parametrize("c", range(N_CASES))
def test_pick_on_the_fixture_tables(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = DevCase128(torch, F)
    nfb = D.nfb
    for qi, q in enumerate(F["qindex"]):
        mse, counted = Table(torch, 2 * nfb * 64, np.uint64, 1, F["mse"][qi]), Table(torch, nfb, np.uint8, 1, F["counted"])
        res, fbs = Table(torch, 21, np.int32, -77), Table(torch, nfb, np.int8, 0x5A)
        hip_ctx.cdef_pick_strengths128_dev(mse.ptr, counted.ptr, F["nhfb"], F["nvfb"], q, F["bd"], res.ptr, fbs.ptr, D.mi, D.mi_stride)
        hip_ctx.synchronize()
        got = fbs.get()
        assert res.get().view(cu.RESULT_DTYPE)[0] == F["result"][qi] and np.array_equal(got, F["fb_strength"][qi]), (c, q, got, F["fb_strength"][qi])
        assert np.array_equal(mse.get().reshape(2, nfb, 64), F["mse"][qi]) and np.array_equal(counted.get(), F["counted"])
    assert D.inputs_untouched()


@pytest.mark.parametrize("c", range(N_CASES))
def test_one_call_search_feeds_the_frame_filter_and_equals_the_stage_split(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = DevCase128(torch, F)
    q = F["qindex"][0]
    hip_ctx.av1_cdef_search128_dev(D.pic, q, D.mse.ptr, D.counted.ptr, D.result.ptr, D.fbs.ptr, D.mi, D.mi_stride, D.work.ptr, bit_depth=D.bd)
    hip_ctx.av1_cdef_frame_dev(D.pic, D.result.ptr, D.fbs.ptr, 0, 3, bit_depth=D.bd)      # the existing frame filter, from the device-side result
    hip_ctx.synchronize()
    mse, counted = D.tables()
    res, fbs = D.picked()
    assert np.array_equal(mse, F["mse"][0]) and np.array_equal(counted, F["counted"])
    assert res == F["result"][0] and np.array_equal(fbs, F["fb_strength"][0]), (fbs, F["fb_strength"][0])
    D.frame_equals(F["out"][0])
    S = DevCase128(torch, F)                                                               # the two stages called one by one
    hip_ctx.av1_cdef_search_mse128_dev(S.pic, q, S.mse.ptr, S.counted.ptr, S.mi, S.mi_stride, S.work.ptr, bit_depth=S.bd)
    hip_ctx.cdef_pick_strengths128_dev(S.mse.ptr, S.counted.ptr, F["nhfb"], F["nvfb"], q, F["bd"], S.result.ptr, S.fbs.ptr, S.mi, S.mi_stride)
    hip_ctx.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(S.tables(), (mse, counted)))
    assert S.picked()[0] == res and np.array_equal(S.picked()[1], fbs) and np.array_equal(S.work.get(), D.work.get())
    assert D.inputs_untouched() and S.inputs_untouched()


@pytest.mark.parametrize("c", range(N_CASES))
def test_frame_filter_on_the_constructed_run(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = DevCase128(torch, F)
    res, fbs = Table(torch, 21, np.int32, -77, F["run_result"][1].reshape(1).view(np.int32)), Table(torch, D.nfb, np.int8, 0x5A, F["run_fb_strength"][1])
    hip_ctx.av1_cdef_frame_dev(D.pic, res.ptr, fbs.ptr, 0, 3, bit_depth=D.bd)
    hip_ctx.synchronize()
    D.frame_equals(F["out"][1])
    res.get(), fbs.get()
    assert D.inputs_untouched()


@pytest.mark.parametrize("bd", (8, 10))
def test_case_d_equals_the_existing_entries(hip_ctx, bd):
    """a grid with nothing 128 wide: byte for byte what the existing entries give on the same picture, both called here"""
    torch = pytest.importorskip("torch")
    F = fixture_case(case_index("D", bd))
    New, Old = DevCase128(torch, F), DevCase128(torch, F)
    for q in F["qindex"]:
        hip_ctx.av1_cdef_search128_dev(New.pic, q, New.mse.ptr, New.counted.ptr, New.result.ptr, New.fbs.ptr, New.mi, New.mi_stride, New.work.ptr, bit_depth=bd)
        hip_ctx.av1_cdef_search_dev(Old.pic, q, Old.mse.ptr, Old.counted.ptr, Old.result.ptr, Old.fbs.ptr, bit_depth=bd)
        New.fresh_out(torch), Old.fresh_out(torch)
        hip_ctx.av1_cdef_frame_dev(New.pic, New.result.ptr, New.fbs.ptr, 0, 3, bit_depth=bd)
        hip_ctx.av1_cdef_frame_dev(Old.pic, Old.result.ptr, Old.fbs.ptr, 0, 3, bit_depth=bd)
        hip_ctx.synchronize()
        assert all(np.array_equal(a, b) for a, b in zip(New.tables(), Old.tables())), q
        assert New.picked()[0] == Old.picked()[0] and np.array_equal(New.picked()[1], Old.picked()[1]), q
        assert New.out.planes()[1] and all(np.array_equal(a, b) for a, b in zip(New.out.planes()[0], Old.out.planes()[0])), q
    # sb_type values above 21 are clamped to 21 (BLOCK_64X16): nothing wide
    odd = np.where(F["sb_type"] == c128.BLOCK_64X64, 200, F["sb_type"]).astype(np.uint8)
    Odd = DevCase128(torch, F, odd)
    hip_ctx.av1_cdef_search128_dev(Odd.pic, F["qindex"][0], Odd.mse.ptr, Odd.counted.ptr, Odd.result.ptr, Odd.fbs.ptr, Odd.mi, Odd.mi_stride, Odd.work.ptr, bit_depth=bd)
    hip_ctx.synchronize()
    assert np.array_equal(Odd.tables()[0], F["mse"][0]) and np.array_equal(Odd.picked()[1], F["fb_strength"][0])


def test_every_new_refusal(hip_ctx):
    torch = pytest.importorskip("torch")
    D, H = DevCase128(torch, fixture_case(case_index("E", 8))), DevCase128(torch, fixture_case(case_index("E", 10)))

    def refused(call, *words):
        with pytest.raises(svtav1_hip.SvtHipError) as e:
            call()
        assert all(w in str(e.value) for w in words), str(e.value)

    def pic(D, **kw):
        F = D.F
        p = svtav1_hip.make_cdef_picture(F["w"], F["h"], D.dbk.ptr, D.dbk.stride, D.pic.d_skip, D.pic.skip_stride, D.src.ptr, D.src.stride, D.out.ptr, D.out.stride)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p

    def search(X, p=None, q=20, mse=0, cnt=0, mi=0, stride=None, work=0, bd=None):
        hip_ctx.av1_cdef_search_mse128_dev(pic(X) if p is None else p, q, X.mse.ptr if mse == 0 else mse, X.counted.ptr if cnt == 0 else cnt,
                                           X.mi if mi == 0 else mi, X.mi_stride if stride is None else stride, X.work.ptr if work == 0 else work,
                                           bit_depth=X.bd if bd is None else bd)

    def whole(X, p=None, q=20, res=0, fbs=0, mi=0, stride=None, work=0, bd=None):
        hip_ctx.av1_cdef_search128_dev(pic(X) if p is None else p, q, X.mse.ptr, X.counted.ptr, X.result.ptr if res == 0 else res, X.fbs.ptr if fbs == 0 else fbs,
                                       X.mi if mi == 0 else mi, X.mi_stride if stride is None else stride, X.work.ptr if work == 0 else work,
                                       bit_depth=X.bd if bd is None else bd)

    def pick(X, mse=0, nh=3, nv=3, q=20, bd=8, res=0, mi=0, stride=None):
        hip_ctx.cdef_pick_strengths128_dev(X.mse.ptr if mse == 0 else mse, X.counted.ptr, nh, nv, q, bd, X.result.ptr if res == 0 else res, X.fbs.ptr,
                                           X.mi if mi == 0 else mi, X.mi_stride if stride is None else stride)

    for f in (search, whole):
        # the new arguments
        refused(lambda: f(D, mi=None), "null")
        refused(lambda: f(D, work=None), "null")
        refused(lambda: f(D, work=D.work.ptr + 4), "aligned")
        refused(lambda: f(D, stride=D.F["w"] // 4 - 1), "mi_stride")
        # what the namesakes refuse
        refused(lambda: f(D, p=pic(D, d_skip=None)), "null")
        refused(lambda: f(D, p=pic(D, source=(1, None))), "null")
        refused(lambda: f(D, p=pic(D, width=60)), "multiple of 8")
        refused(lambda: f(D, p=pic(D, skip_stride=15)), "skip_stride")
        refused(lambda: f(D, p=pic(D, deblocked_stride=(0, 63))), "stride")
        refused(lambda: f(D, q=256), "base_qindex")
        refused(lambda: f(H, bd=12), "10")
        refused(lambda: f(H, p=pic(H, deblocked=(0, H.dbk.ptr[0] + 1))), "aligned")
    refused(lambda: search(D, mse=None), "null")
    refused(lambda: search(D, cnt=None), "null")
    refused(lambda: search(D, mse=D.mse.ptr + 4), "aligned")
    refused(lambda: whole(D, res=None), "null")
    refused(lambda: whole(D, fbs=None), "null")
    refused(lambda: whole(D, res=D.result.ptr + 2), "aligned")
    refused(lambda: pick(D, mi=None), "null")
    refused(lambda: pick(D, stride=32), "mi_stride")          # the first cell of the third fb column is cell 32
    refused(lambda: pick(D, mse=None), "null")
    refused(lambda: pick(D, mse=D.mse.ptr + 4), "aligned")
    refused(lambda: pick(D, res=D.result.ptr + 2), "aligned")
    refused(lambda: pick(D, q=256), "base_qindex")
    refused(lambda: pick(D, bd=12), "bit depth")
    refused(lambda: pick(D, nh=0), "filter blocks")
    refused(lambda: pick(D, nh=128, nv=64), "filter blocks")
    hip_ctx.synchronize()
    for X in (D, H):     # nothing was launched: every output still holds its fill
        assert (X.mse.get() == X.mse.fill).all() and (X.counted.get() == 0x5A).all() and (X.result.get() == -77).all() and (X.fbs.get() == 0x5A).all()
        assert (X.work.get() == X.work.fill).all() and X.inputs_untouched()
