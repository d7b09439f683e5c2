"""GPU: AV1 film-grain synthesis (svthip_film_grain_tables_dev, svthip_av1_[highbd_]add_film_grain_dev) through the C ABI, bit-exact
against the reference's fixture (tests/golden/film_grain.npz: whole planes for some cases, a digest of the reference's planes for every
other) and the restatement (tests/film_grain_util.py).  Every plane sits inside a larger buffer of garbage, source and destination with
different strides, once laid out so that rows move as vectors and once at odd offsets and strides; the whole destination buffer is compared,
so a sample written outside the interior fails the test.  Parameter sets with num_y_points == 0 (film_grain_util.REFERENCE_UNSAFE) are
checked against the restatement alone: the reference must never be run with them (its dealloc_arrays frees a pointer it never allocated)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import film_grain_util as fu  # noqa: E402
import svtav1_hip  # noqa: E402

pytestmark = pytest.mark.gpu

BAD = "80001005"


def _params(p):
    return svtav1_hip.film_grain_params(**{k: v for k, v in p.items()})


class _Planes:
    """the three planes of one picture inside garbage on the device: sources and pre-filled destinations"""

    def __init__(self, torch, planes, bit_depth, aligned, key=0):
        self.torch, self.dt = torch, planes[0].dtype
        rng = np.random.default_rng([7, key, aligned])
        top = (1 << bit_depth) - 1
        self.src, self.dst, self.views = [], [], []
        self.src_stride, self.dst_stride = [], []
        for k, p in enumerate(planes):
            h, w = p.shape
            unit = (4 if k else 8) if aligned else 1
            pad_x, pad_y = (unit if aligned else 3), 2
            ss = (w + 2 * pad_x + 7 + unit - 1) // unit * unit if aligned else w + 7
            ds = ss + (unit if aligned else 2)
            bufs = []
            for stride in (ss, ds):
                b = rng.integers(0, top + 1, (h + 2 * pad_y, stride)).astype(self.dt)
                bufs.append(b)
            bufs[0][pad_y:pad_y + h, pad_x:pad_x + w] = p
            self.views.append((pad_y, pad_x, h, w))
            self.src.append(bufs[0])
            self.dst.append(bufs[1])
            self.src_stride.append(ss)
            self.dst_stride.append(ds)
        as_dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")  # noqa: E731
        self.d_src, self.d_dst = [as_dev(a) for a in self.src], [as_dev(a) for a in self.dst]
        torch.cuda.synchronize()

    def ptrs(self, which):
        bufs, strides = (self.d_src, self.src_stride) if which == "src" else (self.d_dst, self.dst_stride)
        return [t.data_ptr() + (py * s + px) * self.dt.itemsize for t, s, (py, px, _, _) in zip(bufs, strides, self.views)]

    def run(self, ctx, params, w, h, bit_depth, d_tables=None, src=None, dst=None, ss=None, ds=None):
        a = (params, self.ptrs("src") if src is None else src, self.src_stride if ss is None else ss, self.ptrs("dst") if dst is None else dst,
             self.dst_stride if ds is None else ds, w, h)
        if bit_depth == 8:
            ctx.add_film_grain_dev(*a, d_tables)
        else:
            ctx.highbd_add_film_grain_dev(*a, bit_depth, d_tables)
        ctx.synchronize()

    def results(self):
        """[(the whole destination buffer, its interior)] per plane, and the sources as they are now"""
        out = []
        for t, host, (py, px, h, w) in zip(self.d_dst, self.dst, self.views):
            whole = t.cpu().numpy().view(self.dt).reshape(host.shape)
            out.append((whole, whole[py:py + h, px:px + w]))
        return out

    def assert_only_interiors_changed(self, want):
        for k, ((whole, inner), host, (py, px, h, w)) in enumerate(zip(self.results(), self.dst, self.views)):
            assert np.array_equal(inner, want[k]), (k, np.argwhere(inner != want[k])[:6])
            expect = host.copy()
            expect[py:py + h, px:px + w] = want[k]
            assert np.array_equal(whole, expect), ("a sample outside the interior was written", k)
        for t, host in zip(self.d_src, self.src):
            assert np.array_equal(t.cpu().numpy().view(self.dt).reshape(host.shape), host), "a source plane was written"

    def assert_untouched(self):
        for t, host in zip(self.d_dst, self.dst):
            assert np.array_equal(t.cpu().numpy().view(self.dt).reshape(host.shape), host)


def _tables_dev(torch, ctx, p, bd):
    d = torch.full((fu.TABLES_INT16 + 8,), 0x5A5A, dtype=torch.int16, device="cuda:0")
    ctx.film_grain_tables_dev(_params(p), bd, d.data_ptr())
    ctx.synchronize()
    return d


@pytest.mark.parametrize("bd", fu.BIT_DEPTHS)
@pytest.mark.parametrize("s", range(len(fu.PARAM_SETS)))
def test_tables_match_fixture(hip_ctx, s, bd):
    torch = pytest.importorskip("torch")
    got = _tables_dev(torch, hip_ctx, fu.PARAM_SETS[s], bd).cpu().numpy()
    assert (got[fu.TABLES_INT16:] == 0x5A5A).all()
    mine = fu.tables_block(fu.tables_of(s, bd))
    for k, v in fu.split_block(got[:fu.TABLES_INT16]).items():
        assert np.array_equal(v, fu.split_block(mine)[k]), (s, bd, k)
    if s not in fu.REFERENCE_UNSAFE:
        assert np.array_equal(got[:fu.TABLES_INT16], fu.fixture()[f"tables_s{s}_b{bd}"]), (s, bd)


def _check_case(torch, ctx, z, s, bd, aligned, fx):
    w, h = fu.size_of(z)
    p = fu.PARAM_SETS[s]
    planes = fu.source_planes(w, h, bd, s)
    run = _Planes(torch, planes, bd, aligned, key=z * 100 + s)
    run.run(ctx, _params(p), w, h, bd)      # the one-call form
    want = fu.add_film_grain(p, bd, *planes, t=fu.tables_of(s, bd))
    run.assert_only_interiors_changed(want)
    inner = [r[1] for r in run.results()]
    if s not in fu.REFERENCE_UNSAFE:
        assert fu.digest(inner) == fx["digest"][z, s, fu.BIT_DEPTHS.index(bd)], ("differs from the reference", (w, h), s, bd)
        if f"out_z{z}_s{s}_b{bd}_y" in fx:
            for k, a in zip("y cb cr".split(), inner):
                assert np.array_equal(a, fx[f"out_z{z}_s{s}_b{bd}_{k}"]), ((w, h), s, bd, k)


@pytest.mark.parametrize("bd", fu.BIT_DEPTHS)
@pytest.mark.parametrize("z", range(len(fu.SIZES)))
def test_frames_match_reference(hip_ctx, z, bd):
    """every parameter set at this size and depth, rows moved as vectors and sample by sample"""
    torch = pytest.importorskip("torch")
    fx = fu.fixture()
    kept = 0
    for s in range(len(fu.PARAM_SETS)):
        for aligned in (True, False):
            _check_case(torch, hip_ctx, z, s, bd, aligned, fx)
        kept += f"out_z{z}_s{s}_b{bd}_y" in fx
    assert kept >= 1


def test_1080p_matches_reference(hip_ctx):
    torch = pytest.importorskip("torch")
    _check_case(torch, hip_ctx, len(fu.SIZES), fu.BIG_SET, 8, True, fu.fixture())


@pytest.mark.parametrize("bd", fu.BIT_DEPTHS)
def test_given_tables_give_the_same_as_the_one_call_form(hip_ctx, bd):
    torch = pytest.importorskip("torch")
    z, s = 6, 5     # 136x72, lag 3
    w, h = fu.size_of(z)
    p = fu.PARAM_SETS[s]
    planes = fu.source_planes(w, h, bd, s)
    want = fu.add_film_grain(p, bd, *planes, t=fu.tables_of(s, bd))
    d_tables = _tables_dev(torch, hip_ctx, p, bd)
    two = _Planes(torch, planes, bd, True)
    two.run(hip_ctx, _params(p), w, h, bd, d_tables.data_ptr())
    two.assert_only_interiors_changed(want)
    one = _Planes(torch, planes, bd, True)
    one.run(hip_ctx, _params(p), w, h, bd)
    for a, b in zip(one.results(), two.results()):
        assert np.array_equal(a[0], b[0])


@pytest.mark.parametrize("order", ((0, 1), (1, 0)))
def test_two_calls_on_one_context_leave_nothing_stale(order):
    """different seeds, sizes and depths through one context's scratch tables, in both orders"""
    torch = pytest.importorskip("torch")
    calls = ((6, 3, 8), (4, 5, 10))     # 136x72 set 3 at 8 bits; 66x34 set 5 at 10 bits
    ctx = svtav1_hip.Context(0)
    try:
        for i in order + order:
            z, s, bd = calls[i]
            w, h = fu.size_of(z)
            planes = fu.source_planes(w, h, bd, s)
            run = _Planes(torch, planes, bd, False, key=i)
            run.run(ctx, _params(fu.PARAM_SETS[s]), w, h, bd)
            run.assert_only_interiors_changed(fu.add_film_grain(fu.PARAM_SETS[s], bd, *planes, t=fu.tables_of(s, bd)))
    finally:
        ctx.close()


def test_refused_arguments(hip_ctx):
    """the library's error, and nothing launched: destinations and tables keep what they held"""
    torch = pytest.importorskip("torch")
    ctx = hip_ctx
    z, s = 3, 4     # 72x40
    w, h = fu.size_of(z)
    base = fu.PARAM_SETS[s]
    runs = {bd: _Planes(torch, fu.source_planes(w, h, bd, s), bd, True) for bd in fu.BIT_DEPTHS}
    d_tab = torch.full((fu.TABLES_INT16,), 0x5A5A, dtype=torch.int16, device="cuda:0")

    def changed(**kw):
        q = dict(base)
        q.update(kw)
        return _params(q)

    def points(name, pts):
        return changed(**{f"scaling_points_{name}": pts, f"num_{name}_points": len(pts)})

    def coeff(name, i, v):
        c = list(base[f"ar_coeffs_{name}"])
        c[i] = v
        return changed(**{f"ar_coeffs_{name}": c})

    bad_params = [changed(num_y_points=15), changed(num_cb_points=11), changed(num_cr_points=11), changed(num_y_points=-1),
                  points("y", [[10, 5], [10, 9]]), points("cb", [[20, 5], [10, 9]]), points("cr", [[0, 1], [256, 2]]), points("y", [[0, 256]]),
                  changed(scaling_shift=7), changed(scaling_shift=12), changed(ar_coeff_lag=4), changed(ar_coeff_lag=-1), changed(ar_coeff_shift=5),
                  changed(ar_coeff_shift=10), changed(grain_scale_shift=4), changed(grain_scale_shift=-1), coeff("y", 23, 128), coeff("cb", 24, -129),
                  coeff("cr", 0, 200), changed(cb_mult=256), changed(cr_mult=-1), changed(cb_luma_mult=256), changed(cr_luma_mult=256),
                  changed(cb_offset=512), changed(cr_offset=-1)]
    good = _params(base)
    def frame_cases(run, bd):
        src, dst, ss, ds = run.ptrs("src"), run.ptrs("dst"), run.src_stride, run.dst_stride

        def call(**kw):
            run.run(ctx, kw.pop("params", good), kw.pop("w", w), kw.pop("h", h), bd, **kw)

        return [lambda q=q: call(params=q) for q in bad_params] + [
            lambda: call(params=None), lambda: call(src=[None, src[1], src[2]]), lambda: call(dst=[dst[0], dst[1], None]),
            lambda: call(dst=[dst[0], src[1], dst[2]]), lambda: call(w=w + 1), lambda: call(h=h - 1), lambda: call(w=0), lambda: call(h=0),
            lambda: call(ss=[w - 2, ss[1], ss[2]]), lambda: call(ds=[ds[0], ds[1], w // 2 - 1])]

    refused = [c for bd, run in runs.items() for c in frame_cases(run, bd)]
    # a bit depth the entry does not take: the highbd entry with 8 and with 12
    r10 = runs[10]
    for wrong in (8, 12):
        refused.append(lambda b=wrong: ctx.highbd_add_film_grain_dev(good, r10.ptrs("src"), r10.src_stride, r10.ptrs("dst"), r10.dst_stride, w, h, b))
    refused += [lambda: ctx.film_grain_tables_dev(good, 9, d_tab.data_ptr()), lambda: ctx.film_grain_tables_dev(good, 12, d_tab.data_ptr()),
                lambda: ctx.film_grain_tables_dev(None, 8, d_tab.data_ptr()), lambda: ctx.film_grain_tables_dev(good, 8, None)]
    refused += [lambda q=q: ctx.film_grain_tables_dev(q, 10, d_tab.data_ptr()) for q in bad_params]
    for i, call in enumerate(refused):
        with pytest.raises(svtav1_hip.SvtHipError, match=BAD):
            call()
            pytest.fail(f"refusal {i} was accepted")
    ctx.synchronize()
    for run in runs.values():
        run.assert_untouched()
    assert (d_tab.cpu().numpy() == 0x5A5A).all()
    # a NULL context
    lib = svtav1_hip.lib()
    assert lib.svthip_film_grain_tables_dev(None, good, 8, d_tab.data_ptr(), None) & 0xFFFFFFFF == int(BAD, 16)
    r8 = runs[8]
    import ctypes as C
    arr = lambda v, t: (t * 3)(*v)  # noqa: E731
    assert lib.svthip_av1_add_film_grain_dev(None, good, arr(r8.ptrs("src"), C.c_void_p), arr(r8.src_stride, C.c_uint32), arr(r8.ptrs("dst"), C.c_void_p),
                                             arr(r8.dst_stride, C.c_uint32), w, h, None, None) & 0xFFFFFFFF == int(BAD, 16)
