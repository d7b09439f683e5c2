"""GPU: film-grain Wiener denoising (svthip_[highbd_]film_grain_wiener_filter_dev, _dither_dev, _wiener_denoise_dev) through the C ABI
against the reference's fixture (tests/golden/fg_denoise.npz).  No tolerance anywhere: the float planes of the filter stage are compared
over the picture area as uint32 with the numpy restatement's, whose SHA-256 the fixture pins, and every denoised sample equals the one
aom_wiener_denoise_2d wrote.  Every plane sits inside a larger buffer with a stride above its width and the margins of the outputs are
checked.  One chain per picture of fg_model_util: features on the device, numpy's finish, denoising on the device, the noise model on
the device's own denoised planes, against aom_flat_block_finder_run + aom_wiener_denoise_2d + aom_noise_model_update of the reference.
The 2160-row case runs the dither stage alone on float planes made here, against the restatement's serial dither of the same rows."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import fg_denoise_util as du  # noqa: E402
import fg_model_util as mu  # noqa: E402
import svtav1_hip  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0x5A


@pytest.fixture(scope="module")
def expected():
    """per case the restatement's float planes (picture area, uint32) -- computed once, checked against the fixture's digests"""
    fx = du.fixture()
    out = {}
    for k, (p, content, kind) in enumerate(du.CASES):
        w, h, bd = du.PICTURES[p]
        areas = du.picture_area(du.wiener_filter(du.planes_of(p, content), bd, du.psd_of(kind, k)), w, h)
        for c in range(3):
            assert np.array_equal(du.digest(areas[c]), fx[f"result_sha_{k}_{c}"]), ("the restatement no longer gives the fixture's float planes", k, c)
        out[k] = areas
    return out


class _Picture:
    """data planes inside garbage on the device with strides above the widths, output planes filled with FILL"""

    def __init__(self, torch, data, bd, psd):
        self.torch, self.bd = torch, bd
        self.h, self.w = data[0].shape
        rng = np.random.default_rng(5)
        self.keep, self.src, self.src_stride, self.dst, self.dst_stride, self.dst_t = [], [], [], [], [], []
        for k, p in enumerate(data):
            ph, pw = p.shape
            stride = pw + 6 + 2 * k
            buf = rng.integers(0, 1 << bd, (ph + 4, stride)).astype(p.dtype)
            buf[2:2 + ph, 4:4 + pw] = p
            t = torch.from_numpy(buf.view(np.uint8).reshape(-1).copy()).to("cuda:0")
            self.keep.append(t)
            self.src.append(t.data_ptr() + (2 * stride + 4) * p.dtype.itemsize)
            self.src_stride.append(stride)
            dstride = pw + 10 - 2 * k
            d = torch.full(((ph + 2) * dstride * p.dtype.itemsize,), FILL, dtype=torch.uint8, device="cuda:0")
            self.dst_t.append((d, ph, pw, dstride, p.dtype))
            self.dst.append(d.data_ptr() + (dstride + 2) * p.dtype.itemsize)
            self.dst_stride.append(dstride)
        self.psd_t = [torch.from_numpy(np.ascontiguousarray(a[:1024 if c == 0 else 256])).to("cuda:0") for c, a in enumerate(psd)]
        self.psd = [t.data_ptr() for t in self.psd_t]
        self.plane_bytes = svtav1_hip.film_grain_wiener_workspace_bytes(self.w, self.h)
        assert self.plane_bytes == 3 * 4 * int(np.prod(du.result_geometry(self.w, self.h)))
        self.planes = torch.full((self.plane_bytes,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

    def filter(self, ctx, stream=None):
        a = (self.src, self.src_stride, self.w, self.h)
        if self.bd == 8:
            ctx.film_grain_wiener_filter_dev(*a, self.psd, self.planes.data_ptr(), stream=stream)
        else:
            ctx.highbd_film_grain_wiener_filter_dev(*a, self.bd, self.psd, self.planes.data_ptr(), stream=stream)

    def dither(self, ctx, stream=None):
        a = (self.planes.data_ptr(), self.dst, self.dst_stride, self.w, self.h)
        if self.bd == 8:
            ctx.film_grain_dither_dev(*a, stream=stream)
        else:
            ctx.highbd_film_grain_dither_dev(*a, self.bd, stream=stream)

    def denoise(self, ctx, stream=None):
        a = (self.src, self.src_stride, self.dst, self.dst_stride, self.w, self.h)
        if self.bd == 8:
            ctx.film_grain_wiener_denoise_dev(*a, self.psd, stream=stream)
        else:
            ctx.highbd_film_grain_wiener_denoise_dev(*a, self.bd, self.psd, stream=stream)

    def float_planes(self):
        """(picture areas as uint32, True where the margin kept its fill)"""
        pitch, rows = du.result_geometry(self.w, self.h)
        raw = self.planes.cpu().numpy().view(np.uint32).reshape(3, rows, pitch)
        areas, untouched = [], True
        for c in range(3):
            n, pw, ph = 32 >> (c > 0), self.w >> (c > 0), self.h >> (c > 0)
            areas.append(raw[c, n:n + ph, n:n + pw].copy())
            m = raw[c].copy()
            m[n:n + ph, n:n + pw] = 0x5A5A5A5A
            untouched &= bool((m == 0x5A5A5A5A).all())
        return areas, untouched

    def samples(self):
        """the denoised planes; asserts that nothing outside them was written"""
        out = []
        for d, ph, pw, dstride, dt in self.dst_t:
            raw = d.cpu().numpy().view(dt).reshape(ph + 2, dstride)
            out.append(raw[1:1 + ph, 2:2 + pw].copy())
            m = raw.copy()
            m[1:1 + ph, 2:2 + pw] = np.array([FILL, FILL], np.uint8).view(np.uint16)[0] if dt == np.uint16 else FILL
            assert (m.view(np.uint8) == FILL).all(), "written outside a denoised plane"
        return out

    def device_planes(self):
        """(pointers, strides) of the denoised planes, for the noise model"""
        return self.dst, self.dst_stride


def _assert_samples(got, fx, key, what):
    for c in range(3):
        want = fx[f"{key}_{c}"]
        assert np.array_equal(got[c], want), (what, c, np.argwhere(got[c] != want)[:4])


@pytest.mark.parametrize("k", range(len(du.CASES)))
def test_stage_entries_match_reference(hip_ctx, expected, k):
    """the filter's floats as bits, then the dither's samples"""
    torch = pytest.importorskip("torch")
    p, content, kind = du.CASES[k]
    pic = _Picture(torch, du.planes_of(p, content), du.PICTURES[p][2], du.psd_of(kind, k))
    pic.filter(hip_ctx)
    hip_ctx.synchronize()
    areas, untouched = pic.float_planes()
    for c in range(3):
        assert np.array_equal(areas[c], expected[k][c]), (du.CASES[k], c, np.argwhere(areas[c] != expected[k][c])[:4])
    assert untouched, "the filter wrote outside the picture area"
    pic.dither(hip_ctx)
    hip_ctx.synchronize()
    _assert_samples(pic.samples(), du.fixture(), f"den_{k}", du.CASES[k])


@pytest.mark.parametrize("k", range(len(du.CASES)))
def test_one_call_matches_reference(hip_ctx, k):
    torch = pytest.importorskip("torch")
    p, content, kind = du.CASES[k]
    pic = _Picture(torch, du.planes_of(p, content), du.PICTURES[p][2], du.psd_of(kind, k))
    pic.denoise(hip_ctx)
    hip_ctx.synchronize()
    _assert_samples(pic.samples(), du.fixture(), f"den_{k}", du.CASES[k])


def test_small_large_small_on_one_context_leaves_nothing_stale():
    """different sizes and depths through one context's scratch, which grows and is reused"""
    torch = pytest.importorskip("torch")
    ctx = svtav1_hip.Context(0)
    try:
        for k in (10, 4, 10, 7, 0, 4):
            p, content, kind = du.CASES[k]
            pic = _Picture(torch, du.planes_of(p, content), du.PICTURES[p][2], du.psd_of(kind, k))
            pic.denoise(ctx)
            ctx.synchronize()
            _assert_samples(pic.samples(), du.fixture(), f"den_{k}", k)
    finally:
        ctx.close()


def test_caller_stream(hip_ctx, expected):
    """both forms on a stream of the caller's, the stage entries one behind the other without a host wait between them"""
    torch = pytest.importorskip("torch")
    k = 5
    p, content, kind = du.CASES[k]
    s = torch.cuda.Stream(device="cuda:0")
    staged = _Picture(torch, du.planes_of(p, content), du.PICTURES[p][2], du.psd_of(kind, k))
    whole = _Picture(torch, du.planes_of(p, content), du.PICTURES[p][2], du.psd_of(kind, k))
    staged.filter(hip_ctx, stream=s.cuda_stream)
    staged.dither(hip_ctx, stream=s.cuda_stream)
    whole.denoise(hip_ctx, stream=s.cuda_stream)
    s.synchronize()
    areas, _ = staged.float_planes()
    for c in range(3):
        assert np.array_equal(areas[c], expected[k][c])
    _assert_samples(staged.samples(), du.fixture(), f"den_{k}", "staged")
    _assert_samples(whole.samples(), du.fixture(), f"den_{k}", "one call")


@pytest.mark.parametrize("p", range(len(mu.PICTURES)))
def test_chain_features_denoise_model_matches_reference(hip_ctx, p):
    """device features, numpy's finish, device denoising, device noise model on the device's own denoised planes"""
    torch = pytest.importorskip("torch")
    fx = du.fixture()
    w, h, bd = mu.PICTURES[p]
    data = mu.planes_of(p)[0]
    pic = _Picture(torch, data, bd, du.psd_of("default"))
    nb = int(np.prod(mu.blocks_of(w, h)))
    d_feat = torch.zeros(nb * mu.FEATURES.itemsize, dtype=torch.uint8, device="cuda:0")
    d_is = torch.zeros(nb, dtype=torch.uint8, device="cuda:0")
    if bd == 8:
        hip_ctx.film_grain_flat_block_features_dev(pic.src[0], pic.src_stride[0], w, h, d_feat.data_ptr(), d_is.data_ptr())
    else:
        hip_ctx.highbd_film_grain_flat_block_features_dev(pic.src[0], pic.src_stride[0], w, h, bd, d_feat.data_ptr(), d_is.data_ptr())
    pic.denoise(hip_ctx)
    hip_ctx.synchronize()
    final, _, _ = mu.finish_flat_blocks(np.frombuffer(d_feat.cpu().numpy().tobytes(), mu.FEATURES), d_is.cpu().numpy())
    assert np.array_equal(final, fx[f"chain_map_{p}"])
    _assert_samples(pic.samples(), fx, f"chain_den_{p}", ("chain", p))
    # the noise model reads data and denoised planes with one stride per plane: the denoised planes go into buffers of the data's strides
    den_t, den_ptr = [], []
    for c, (d, ph, pw, dstride, dt) in enumerate(pic.dst_t):
        stride = pic.src_stride[c]
        buf = torch.full((ph * stride * np.dtype(dt).itemsize,), FILL, dtype=torch.uint8, device="cuda:0")
        src = d.view(torch.int16 if dt == np.uint16 else torch.uint8).reshape(ph + 2, dstride)[1:1 + ph, 2:2 + pw]
        buf.view(torch.int16 if dt == np.uint16 else torch.uint8).reshape(ph, stride)[:, :pw] = src   # a device copy
        den_t.append(buf)
        den_ptr.append(buf.data_ptr())
    d_flat = torch.from_numpy(final.copy()).to("cuda:0")
    d_state = torch.zeros(mu.STATE.itemsize, dtype=torch.uint8, device="cuda:0")
    if bd == 8:
        hip_ctx.film_grain_noise_model_dev(pic.src, den_ptr, pic.src_stride, w, h, d_flat.data_ptr(), d_state.data_ptr())
    else:
        hip_ctx.highbd_film_grain_noise_model_dev(pic.src, den_ptr, pic.src_stride, w, h, bd, d_flat.data_ptr(), d_state.data_ptr())
    hip_ctx.synchronize()
    assert d_state.cpu().numpy().tobytes() == fx[f"chain_{p}"].tobytes(), ("the state of the chain differs from the reference's", p)


def test_dither_of_2160_rows_hands_errors_from_band_to_band(hip_ctx):
    """34 bands of 64 rows and a last one of 48 on a narrow picture (the dither does not care where the floats come from): float planes
    made here, with values below 0 and above 1, against the restatement's serial dither"""
    torch = pytest.importorskip("torch")
    w, h, bd = 36, 2160, 8
    pitch, rows = du.result_geometry(w, h)
    rng = np.random.default_rng(77)
    planes = (rng.random((3, rows, pitch)) * 1.2 - 0.1).astype(np.float32)
    want = du.dither([planes[c].copy() for c in range(3)], w, h, bd)
    pic = _Picture(torch, [np.zeros((h >> (c > 0), w >> (c > 0)), np.uint8) for c in range(3)], bd, du.psd_of("zero"))
    pic.planes = torch.from_numpy(planes.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    pic.dither(hip_ctx)
    hip_ctx.synchronize()
    got = pic.samples()
    for c in range(3):
        assert np.array_equal(got[c], want[c]), (c, np.argwhere(got[c] != want[c])[:4])
