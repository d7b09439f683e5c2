"""GPU: the CDEF entries bit-exact against the reference's fixture (tests/golden/cdef.npz): the tables and counted flags of the strength
search for every case and base_qindex, the pick on the fixture's tables and on the constructed tie tables, the search end to end, the frame
filter for every recorded run and fed from the search's device-side result with no host copy in between, dist_8x8 on all block pairs, the
chain into the loop-restoration frame filter, and every refusal.  Planes sit inside larger allocations with an odd guard of pattern
samples that must come back untouched, tables between guard words; inputs must come back unchanged.  Every comparison is equality.
The shapes are the fixture's: one fb; 4 x 3 and 3 x 4 fbs with an 8-wide last column and an 8-high last row; an fb with a single listed
block; an fb entirely skipped.  A tensor that torch fills is handed to an entry only after _ready() (tests/lr_gpu_util.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import cdef_util as cu  # noqa: E402
import svtav1_hip  # noqa: E402
from lr_gpu_util import FILL, Guarded, _dev, _ready  # noqa: E402
from test_cdef_vs_ref import N_CASES, fixture, fixture_case  # noqa: E402

pytestmark = pytest.mark.gpu
SKIP_GUARD = 3


class Table:
    """a device array between two guard elements"""

    def __init__(self, torch, n, dtype, fill, host=None):
        a = np.full(n + 2, fill, dtype)
        if host is not None:
            a[1:-1] = np.asarray(host, dtype).reshape(-1)
        self.fill, self.dtype, self.dev = a[0], np.dtype(dtype), _dev(torch, a)
        self.ptr = self.dev.data_ptr() + self.dtype.itemsize

    def get(self):
        a = self.dev.cpu().numpy().view(self.dtype)
        assert a[0] == self.fill and a[-1] == self.fill, "an entry wrote outside its table"
        return a[1:-1].copy()


class DevCase:
    """a fixture case on the device: guarded deblocked, source and output planes, the skip map inside a guard of skipped cells, tables"""

    def __init__(self, torch, F):
        self.F, self.bd, self.nfb = F, F["bd"], F["nhfb"] * F["nvfb"]
        self.dbk, self.src = Guarded(torch, F["dbk"], F["bd"]), Guarded(torch, F["src"], F["bd"])
        self.out = Guarded(torch, [np.full_like(p, 7) for p in F["dbk"]], F["bd"])
        sk = np.ones((F["skip"].shape[0] + 2, F["skip"].shape[1] + SKIP_GUARD), np.uint8)
        sk[1:-1, 1:1 + F["skip"].shape[1]] = F["skip"]
        self.skip_host, self.skip = sk, _dev(torch, sk)
        self.pic = svtav1_hip.make_cdef_picture(F["w"], F["h"], self.dbk.ptr, self.dbk.stride, self.skip.data_ptr() + sk.shape[1] + 1, sk.shape[1],
                                                self.src.ptr, self.src.stride, self.out.ptr, self.out.stride)
        self.mse = Table(torch, 2 * self.nfb * 64, np.uint64, 0x5A5A5A5A5A5A5A5A)
        self.counted = Table(torch, self.nfb, np.uint8, 0x5A)
        self.result = Table(torch, 21, np.int32, -77)
        self.fbs = Table(torch, self.nfb, np.int8, 0x5A)

    def inputs_untouched(self):
        ok = np.array_equal(self.skip.cpu().numpy().reshape(self.skip_host.shape), self.skip_host)
        for g, k in ((self.dbk, "dbk"), (self.src, "src")):
            planes, guard = g.planes()
            ok &= guard and all(np.array_equal(a, b) for a, b in zip(planes, self.F[k]))
        return bool(ok)

    def tables(self):
        return self.mse.get().reshape(2, self.nfb, 64), self.counted.get()

    def picked(self):
        return self.result.get().view(cu.RESULT_DTYPE)[0], self.fbs.get()

    def fresh_out(self, torch):
        self.out = Guarded(torch, [np.full_like(p, 7) for p in self.F["dbk"]], self.bd)
        for p in range(3):
            self.pic.out[p], self.pic.out_stride[p] = self.out.ptr[p], self.out.stride[p]

    def frame_equals(self, want, planes=(0, 1, 2)):
        got, guard = self.out.planes()
        assert guard, "the frame filter wrote outside its planes"
        for p in range(3):
            assert np.array_equal(got[p], want[p] if p in planes else np.full_like(want[p], 7)), p


@pytest.mark.parametrize("c", range(N_CASES))
def test_search_tables_and_counted_flags(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = DevCase(torch, F)
    for qi, q in enumerate(F["qindex"]):
        hip_ctx.av1_cdef_search_mse_dev(D.pic, q, D.mse.ptr, D.counted.ptr, bit_depth=D.bd)
        hip_ctx.synchronize()
        mse, counted = D.tables()
        assert np.array_equal(counted, F["counted"]), (c, q)
        assert np.array_equal(mse, F["mse"][qi]), (c, q, np.argwhere(mse != F["mse"][qi])[:8])
    assert D.inputs_untouched()
    assert D.out.planes()[1] and all((p == 7).all() for p in D.out.planes()[0]), "a search entry wrote a picture"


@pytest.mark.parametrize("c", range(N_CASES))
def test_pick_on_the_fixture_tables(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    nfb = F["nhfb"] * F["nvfb"]
    for qi, q in enumerate(F["qindex"]):
        mse, counted = Table(torch, 2 * nfb * 64, np.uint64, 1, F["mse"][qi]), Table(torch, nfb, np.uint8, 1, F["counted"])
        res, fbs = Table(torch, 21, np.int32, -77), Table(torch, nfb, np.int8, 0x5A)
        hip_ctx.cdef_pick_strengths_dev(mse.ptr, counted.ptr, F["nhfb"], F["nvfb"], q, F["bd"], res.ptr, fbs.ptr)
        hip_ctx.synchronize()
        assert res.get().view(cu.RESULT_DTYPE)[0] == F["result"][qi] and np.array_equal(fbs.get(), F["fb_strength"][qi]), (c, q)
        assert np.array_equal(mse.get().reshape(2, nfb, 64), F["mse"][qi]) and np.array_equal(counted.get(), F["counted"])


def test_pick_on_the_constructed_tie_tables(hip_ctx):
    torch = pytest.importorskip("torch")
    z = fixture()
    want = z["syn_result"].view(cu.RESULT_DTYPE).reshape(-1)
    nfb = z["syn_counted"].shape[1]
    for t in range(len(z["syn_qindex"])):
        mse, counted = Table(torch, 2 * nfb * 64, np.uint64, 1, z["syn_mse"][t]), Table(torch, nfb, np.uint8, 1, z["syn_counted"][t])
        res, fbs = Table(torch, 21, np.int32, -77), Table(torch, nfb, np.int8, 0x5A)
        hip_ctx.cdef_pick_strengths_dev(mse.ptr, counted.ptr, 3, 2, int(z["syn_qindex"][t]), 8, res.ptr, fbs.ptr)
        hip_ctx.synchronize()
        assert res.get().view(cu.RESULT_DTYPE)[0] == want[t] and np.array_equal(fbs.get(), z["syn_fb_strength"][t]), t


@pytest.mark.parametrize("c", range(N_CASES))
def test_search_end_to_end_feeds_the_frame_filter_on_the_device(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = DevCase(torch, F)
    q = F["qindex"][0]
    hip_ctx.av1_cdef_search_dev(D.pic, q, D.mse.ptr, D.counted.ptr, D.result.ptr, D.fbs.ptr, bit_depth=D.bd)
    hip_ctx.av1_cdef_frame_dev(D.pic, D.result.ptr, D.fbs.ptr, 0, 3, bit_depth=D.bd)      # from the device-side result, no host copy in between
    hip_ctx.synchronize()
    mse, counted = D.tables()
    res, fbs = D.picked()
    assert np.array_equal(mse, F["mse"][0]) and np.array_equal(counted, F["counted"])
    assert res == F["result"][0] and np.array_equal(fbs, F["fb_strength"][0])
    D.frame_equals(F["out"][0])
    assert D.inputs_untouched()


@pytest.mark.parametrize("c", range(N_CASES))
def test_frame_filter_for_every_recorded_run(hip_ctx, c):
    torch = pytest.importorskip("torch")
    F = fixture_case(c)
    D = DevCase(torch, F)
    for r in range(len(F["run_result"])):
        res, fbs = Table(torch, 21, np.int32, -77, F["run_result"][r].reshape(1).view(np.int32)), Table(torch, D.nfb, np.int8, 0x5A, F["run_fb_strength"][r])
        for planes in (((0, 3), (1, 3)) if r == 1 else ((0, 3),)):
            D.fresh_out(torch)
            hip_ctx.av1_cdef_frame_dev(D.pic, res.ptr, fbs.ptr, planes[0], planes[1], bit_depth=D.bd)
            hip_ctx.synchronize()
            D.frame_equals(F["out"][r], range(*planes))
        res.get(), fbs.get()
    D.fresh_out(torch)
    hip_ctx.av1_cdef_frame_dev(D.pic, res.ptr, fbs.ptr, 2, 2, bit_depth=D.bd)              # an empty range of planes writes nothing
    hip_ctx.synchronize()
    D.frame_equals(F["out"][0], ())
    assert D.inputs_untouched()


def test_frame_filter_looks_only_at_the_planes_it_works_on(hip_ctx):
    """luma alone with no chroma plane given; chroma alone with no luma output; never a source plane"""
    torch = pytest.importorskip("torch")
    F = fixture_case(4)
    D = DevCase(torch, F)
    res, fbs = Table(torch, 21, np.int32, -77, F["run_result"][1].reshape(1).view(np.int32)), Table(torch, D.nfb, np.int8, 0x5A, F["run_fb_strength"][1])
    for planes in ((0, 1), (1, 3)):
        D.fresh_out(torch)
        keep = [p in range(*planes) for p in range(3)]
        pic = svtav1_hip.make_cdef_picture(F["w"], F["h"], [D.dbk.ptr[p] if keep[p] or p == 0 else None for p in range(3)], D.dbk.stride, D.pic.d_skip,
                                           D.pic.skip_stride, out=[D.out.ptr[p] if keep[p] else None for p in range(3)], out_stride=D.out.stride)
        hip_ctx.av1_cdef_frame_dev(pic, res.ptr, fbs.ptr, planes[0], planes[1], bit_depth=D.bd)
        hip_ctx.synchronize()
        D.frame_equals(F["out"][1], range(*planes))
    assert D.inputs_untouched()


@pytest.mark.parametrize("bd", (8, 10))
def test_dist_8x8_on_all_pairs(hip_ctx, bd):
    torch = pytest.importorskip("torch")
    z = fixture()
    d, s, want = z[f"dist{bd}_dst"], z[f"dist{bd}_src"], z[f"dist{bd}_ref"]
    n = len(want)
    dd, ds, out = Table(torch, n * 64, np.uint16, 9, d), Table(torch, n * 64, np.uint16, 9, s), Table(torch, n, np.uint64, 0x5A5A)
    hip_ctx.cdef_dist_8x8_batch_dev(dd.ptr, ds.ptr, n, bd - 8, out.ptr)
    hip_ctx.synchronize()
    got = out.get()
    assert np.array_equal(got, want), (bd, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])


def test_chain_into_loop_restoration(hip_ctx):
    """cdef_frame_dev's output handed as svthip_lr_picture.cdef to the loop-restoration frame filter with every unit RESTORE_NONE"""
    torch = pytest.importorskip("torch")
    F = fixture_case(0)
    D = DevCase(torch, F)
    res, fbs = Table(torch, 21, np.int32, -77, F["run_result"][1].reshape(1).view(np.int32)), Table(torch, D.nfb, np.int8, 0x5A, F["run_fb_strength"][1])
    hip_ctx.av1_cdef_frame_dev(D.pic, res.ptr, fbs.ptr, 0, 3, bit_depth=D.bd)
    lr = svtav1_hip.make_lr_picture(F["w"], F["h"], D.out.ptr, D.out.stride, D.dbk.ptr, D.dbk.stride)
    restored = Guarded(torch, [np.full_like(p, 9) for p in F["dbk"]], D.bd)
    n_units = svtav1_hip.lr_unit_geometry(F["w"], F["h"])[0][3]
    types = torch.zeros(n_units, dtype=torch.uint8, device="cuda:0")
    _ready(torch)
    hip_ctx.av1_lr_filter_frame_dev(lr, restored.ptr, restored.stride, 0, 3, types.data_ptr(), None, None, bit_depth=D.bd)
    hip_ctx.synchronize()
    got, guard = restored.planes()
    assert guard and all(np.array_equal(got[p], F["out"][1][p]) for p in range(3))
    assert any(not np.array_equal(F["out"][1][p], F["dbk"][p]) for p in range(3))
    D.frame_equals(F["out"][1])


def test_every_refusal(hip_ctx):
    torch = pytest.importorskip("torch")
    F8, F10 = fixture_case(0), fixture_case(3)
    D, H = DevCase(torch, F8), DevCase(torch, F10)

    def refused(call, *words):
        with pytest.raises(svtav1_hip.SvtHipError) as e:
            call()
        assert all(w in str(e.value) for w in words), str(e.value)

    def pic(D, **kw):
        F = D.F
        p = svtav1_hip.make_cdef_picture(F["w"], F["h"], D.dbk.ptr, D.dbk.stride, D.pic.d_skip, D.pic.skip_stride, D.src.ptr, D.src.stride, D.out.ptr,
                                         D.out.stride)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p

    search = lambda p, q=20, mse=D.mse.ptr, cnt=D.counted.ptr: hip_ctx.av1_cdef_search_mse_dev(p, q, mse, cnt)                      # noqa: E731
    whole = lambda p, q=20, res=D.result.ptr, fbs=D.fbs.ptr: hip_ctx.av1_cdef_search_dev(p, q, D.mse.ptr, D.counted.ptr, res, fbs)   # noqa: E731
    frame = lambda p, ps=0, pe=3, res=D.result.ptr, fbs=D.fbs.ptr: hip_ctx.av1_cdef_frame_dev(p, res, fbs, ps, pe)                   # noqa: E731
    # null pointers
    refused(lambda: search(None), "null")
    for k in ("deblocked", "source"):
        refused(lambda: search(pic(D, **{k: (1, None)})), "null")
    refused(lambda: search(pic(D, d_skip=None)), "null")
    refused(lambda: search(pic(D), mse=None), "null")
    refused(lambda: search(pic(D), cnt=None), "null")
    refused(lambda: whole(pic(D), res=None), "null")
    refused(lambda: whole(pic(D), fbs=None), "null")
    refused(lambda: frame(pic(D, out=(2, None))), "null")
    refused(lambda: frame(pic(D), res=None), "null")
    refused(lambda: frame(pic(D), fbs=None), "null")
    refused(lambda: hip_ctx.cdef_pick_strengths_dev(None, D.counted.ptr, 1, 1, 20, 8, D.result.ptr, D.fbs.ptr), "null")
    refused(lambda: hip_ctx.cdef_dist_8x8_batch_dev(None, D.mse.ptr, 1, 0, D.mse.ptr), "null")
    # sizes
    for k, v in (("width", 0), ("height", 0), ("width", 60), ("height", 68)):
        refused(lambda: search(pic(D, **{k: v})), "multiple of 8")
        refused(lambda: frame(pic(D, **{k: v})), "multiple of 8")
    # strides
    refused(lambda: search(pic(D, deblocked_stride=(0, 63))), "stride")
    refused(lambda: search(pic(D, source_stride=(2, 31))), "stride")
    refused(lambda: search(pic(D, skip_stride=15)), "skip_stride")
    refused(lambda: frame(pic(D, out_stride=(1, 31))), "stride")
    # an output plane over a deblocked plane
    refused(lambda: frame(pic(D, out=(0, D.dbk.ptr[0] + 64 * 3))), "overlaps")
    refused(lambda: frame(pic(D, out=(1, D.dbk.ptr[2]))), "overlaps")
    # base_qindex, bit depth
    refused(lambda: search(pic(D), q=256), "base_qindex")
    refused(lambda: whole(pic(D), q=256), "base_qindex")
    refused(lambda: hip_ctx.cdef_pick_strengths_dev(D.mse.ptr, D.counted.ptr, 1, 1, 256, 8, D.result.ptr, D.fbs.ptr), "base_qindex")
    refused(lambda: hip_ctx.cdef_pick_strengths_dev(D.mse.ptr, D.counted.ptr, 1, 1, 20, 12, D.result.ptr, D.fbs.ptr), "bit depth")
    refused(lambda: hip_ctx.av1_cdef_search_mse_dev(pic(H), 20, H.mse.ptr, H.counted.ptr, bit_depth=12), "10")
    refused(lambda: hip_ctx.av1_cdef_search_dev(pic(H), 20, H.mse.ptr, H.counted.ptr, H.result.ptr, H.fbs.ptr, bit_depth=12), "10")
    refused(lambda: hip_ctx.av1_cdef_frame_dev(pic(H), H.result.ptr, H.fbs.ptr, 0, 3, bit_depth=12), "10")
    # misaligned 16-bit planes and 64-bit tables
    refused(lambda: hip_ctx.av1_cdef_search_mse_dev(pic(H, deblocked=(0, H.dbk.ptr[0] + 1)), 20, H.mse.ptr, H.counted.ptr, bit_depth=10), "aligned")
    refused(lambda: hip_ctx.av1_cdef_search_mse_dev(pic(H, source=(1, H.src.ptr[1] + 1)), 20, H.mse.ptr, H.counted.ptr, bit_depth=10), "aligned")
    refused(lambda: hip_ctx.av1_cdef_frame_dev(pic(H, out=(2, H.out.ptr[2] + 1)), H.result.ptr, H.fbs.ptr, 0, 3, bit_depth=10), "aligned")
    refused(lambda: search(pic(D), mse=D.mse.ptr + 4), "aligned")
    refused(lambda: hip_ctx.cdef_pick_strengths_dev(D.mse.ptr + 4, D.counted.ptr, 1, 1, 20, 8, D.result.ptr, D.fbs.ptr), "aligned")
    refused(lambda: hip_ctx.cdef_pick_strengths_dev(D.mse.ptr, D.counted.ptr, 1, 1, 20, 8, D.result.ptr + 2, D.fbs.ptr), "aligned")
    refused(lambda: hip_ctx.cdef_dist_8x8_batch_dev(D.mse.ptr, D.mse.ptr, 1, 0, D.mse.ptr + 4), "aligned")
    # plane ranges, the pick's size, the shift
    refused(lambda: frame(pic(D), ps=2, pe=1), "planes")
    refused(lambda: frame(pic(D), ps=0, pe=4), "planes")
    refused(lambda: hip_ctx.cdef_pick_strengths_dev(D.mse.ptr, D.counted.ptr, 0, 1, 20, 8, D.result.ptr, D.fbs.ptr), "filter blocks")
    refused(lambda: hip_ctx.cdef_pick_strengths_dev(D.mse.ptr, D.counted.ptr, 128, 64, 20, 8, D.result.ptr, D.fbs.ptr), "filter blocks")
    refused(lambda: hip_ctx.cdef_dist_8x8_batch_dev(D.mse.ptr, D.mse.ptr, 1, 3, D.mse.ptr), "coeff_shift")
    hip_ctx.synchronize()
    # nothing was launched: every output still holds its fill
    for X in (D, H):
        assert (X.mse.get() == X.mse.fill).all() and (X.counted.get() == 0x5A).all() and (X.result.get() == -77).all() and (X.fbs.get() == 0x5A).all()
        assert X.out.planes()[1] and all((p == 7).all() for p in X.out.planes()[0]) and X.inputs_untouched()
    assert FILL[8] != 7
