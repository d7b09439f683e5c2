"""GPU: input-picture noise detection and denoising (svthip_pa_noise_detect_dev, svthip_pa_denoise_dev) through the C ABI, bit-exact against
the reference's fixture (tests/golden/pa_noise.npz) and the restatement (tests/pa_noise_util.py).  The pool holds picture interiors only:
every other byte of it, the luma borders included, is 0xEE and svthip_pa_derive_planes_dev is not run before the entries under test, as in
the real call sequence.  The chroma planes lie at offsets 2 past a multiple of 4 with stride w/2 + 2."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import pa_noise_util as nu  # noqa: E402
import pa_stats_util as pu  # noqa: E402
import svtav1_hip  # noqa: E402
from svtav1_hip import synth  # noqa: E402

pytestmark = pytest.mark.gpu

FILL8, FILL32, FILL64 = 0xAA, -1431655766, -6148914691236517206


def _pool(planes):
    """planes: [(luma, cb, cr)] of one size -> (pool of 0xEE with the interiors in it, descriptors, chroma offsets, chroma stride)"""
    laid_out, descs = svtav1_hip.build_picture_pool([synth.PaPicture(luma) for luma, _, _ in planes])
    h, w = planes[0][0].shape
    cstride = w // 2 + 2
    luma_bytes = laid_out.size + (-laid_out.size) % 4 + 2   # chroma starts 2 past a multiple of 4
    pool = np.full(luma_bytes + len(planes) * 2 * cstride * (h // 2) + 256, 0xEE, np.uint8)
    offsets, at = [], luma_bytes
    for (luma, cb, cr), d in zip(planes, descs):
        _luma_view(pool, d, w, h)[:] = luma
        pair = []
        for c in (cb, cr):
            _chroma_view(pool, at, cstride, w, h)[:] = c
            pair.append(at)
            at += cstride * (h // 2)
        offsets.append(pair)
    return pool, descs, offsets, cstride


def _luma_view(pool, d, w, h):
    return pool[d.full_offset:d.full_offset + d.full_stride * (h + 136)].reshape(h + 136, d.full_stride)[68:68 + h, 68:68 + w]


def _chroma_view(pool, at, cstride, w, h):
    return pool[at:at + cstride * (h // 2)].reshape(h // 2, cstride)[:, :w // 2]


class _Run:
    """the pictures of one launch on the device, the outputs pre-filled"""

    def __init__(self, torch, ctx, planes, write=True, s=None):
        self.torch, self.ctx, self.planes, self.s = torch, ctx, planes, s
        self.stream = s.cuda_stream if s is not None else None
        self.pool, self.descs, self.offsets, self.cstride = _pool(planes)
        self.h, self.w = planes[0][0].shape
        self.n, self.n_sb = len(planes), pu.sb_grid(self.w, self.h)[0] * pu.sb_grid(self.w, self.h)[1]
        self.dstride = self.w + 8
        dev = "cuda:0"
        self.d_pool = torch.from_numpy(self.pool).to(dev)
        self.d_den = torch.full((self.n, self.h, self.dstride), FILL8, dtype=torch.uint8, device=dev) if write else None
        self.d_var = torch.full((self.n, self.n_sb, 2), FILL64, dtype=torch.int64, device=dev)
        self.d_flat = torch.full((self.n, self.n_sb), FILL8, dtype=torch.uint8, device=dev)
        self.d_pic = torch.full((self.n, 4), FILL32, dtype=torch.int32, device=dev)
        if s is None:
            torch.cuda.synchronize()
        else:
            s.wait_stream(torch.cuda.current_stream())   # stream order behind the upload and the fills, not a host wait

    def _wait(self):
        """the context's stream, or the caller's stream alone when the run has one"""
        if self.s is None:
            self.ctx.synchronize()
        else:
            self.s.synchronize()

    def detect(self, sub):
        self.ctx.pa_noise_detect_dev(self.d_pool.data_ptr(), self.descs, sub, self.d_den.data_ptr() if self.d_den is not None else None, self.dstride,
                                     self.d_var.data_ptr(), self.d_flat.data_ptr(), self.d_pic.data_ptr(), stream=self.stream)
        self._wait()
        out = {"sb_var": self.d_var.cpu().numpy().view(np.uint64), "flat_noise": self.d_flat.cpu().numpy(), "picture": self.d_pic.cpu().numpy().view(np.uint32)}
        if self.d_den is not None:
            out["denoised"] = self.d_den.cpu().numpy()
        return out

    def denoise(self):
        self.ctx.pa_denoise_dev(self.d_pool.data_ptr(), self.descs, self.offsets, self.cstride, self.d_den.data_ptr(), self.dstride, self.d_flat.data_ptr(),
                                self.d_pic.data_ptr(), stream=self.stream)
        self._wait()
        return self.d_pool.cpu().numpy()

    def expected_pool(self, outs):
        """the pool as uploaded with the three interiors of every picture replaced by outs[i] = (luma, cb, cr)"""
        want = self.pool.copy()
        for d, pair, (luma, cb, cr) in zip(self.descs, self.offsets, outs):
            _luma_view(want, d, self.w, self.h)[:] = luma
            _chroma_view(want, pair[0], self.cstride, self.w, self.h)[:] = cb
            _chroma_view(want, pair[1], self.cstride, self.w, self.h)[:] = cr
        return want


@pytest.mark.parametrize("sub", (0, 1))
@pytest.mark.parametrize("c", range(len(nu.CASES)))
def test_detection_matches_fixture(hip_ctx, c, sub):
    """every picture of a case in one launch, with d_denoised"""
    torch = pytest.importorskip("torch")
    w, h, pics = nu.fixture_cases()[c]
    run = _Run(torch, hip_ctx, [p[:3] for p in pics])
    got = run.detect(sub)
    complete = pu.complete_sbs(w, h)
    for i, (luma, cb, cr, outs) in enumerate(pics):
        mine = nu.detect(luma, sub)
        for k in nu.DETECT_OUTPUTS:
            assert np.array_equal(got[k][i], outs[sub][k]) and np.array_equal(mine[k], outs[sub][k]), ((w, h), i, sub, k)
        # the outputs were pre-filled: the slots of incomplete SBs were written, as zeros
        assert (got["flat_noise"][i][~complete] == 0).all() and (got["sb_var"][i][~complete] == 0).all()
        # the denoised luma of the whole picture, incomplete SBs included, and not a byte past `width`
        assert np.array_equal(got["denoised"][i][:, :w], outs[sub]["denoised"]) and np.array_equal(mine["denoised"], outs[sub]["denoised"]), ((w, h), i, sub)
        assert (got["denoised"][i][:, w:] == FILL8).all()
    assert np.array_equal(run.d_pool.cpu().numpy(), run.pool)      # detection writes nothing into the pool


@pytest.mark.parametrize("sub", (0, 1))
def test_detection_only_gives_the_same(hip_ctx, sub):
    torch = pytest.importorskip("torch")
    w, h, pics = nu.fixture_cases()[4]      # 200x136
    got = _Run(torch, hip_ctx, [p[:3] for p in pics], write=False).detect(sub)
    for i, (_, _, _, outs) in enumerate(pics):
        for k in nu.DETECT_OUTPUTS:
            assert np.array_equal(got[k][i], outs[sub][k]), (i, sub, k)


def test_batch_of_three_equals_three_single_launches(hip_ctx):
    torch = pytest.importorskip("torch")
    w, h, pics = nu.fixture_cases()[4]      # 200x136
    three = [pics[i][:3] for i in (1, 3, 5)]   # mixed, class 3, clamped
    batch = _Run(torch, hip_ctx, three).detect(1)
    for i, planes in enumerate(three):
        single = _Run(torch, hip_ctx, [planes]).detect(1)
        for k in batch:
            assert np.array_equal(batch[k][i], single[k][0]), (i, k)


@pytest.mark.parametrize("c", (1, 4))       # 136x72, 200x136
def test_denoise_takes_each_arm_and_touches_nothing_else(hip_ctx, c):
    """all pictures of the case in one launch: nothing, the flat SBs, the whole picture, chosen on the device.  The whole pool is compared:
    samples outside the arm's reach and every border and padding byte keep what was uploaded"""
    torch = pytest.importorskip("torch")
    w, h, pics = nu.fixture_cases()[c]
    sub = 1
    assert {nu.arm(p[3][sub]["picture"]) for p in pics} == set(nu.ARMS)
    run = _Run(torch, hip_ctx, [p[:3] for p in pics])
    run.detect(sub)
    after = run.denoise()
    want = run.expected_pool([(p[3][sub]["out_luma"], p[3][sub]["out_cb"], p[3][sub]["out_cr"]) for p in pics])
    for i, (d, pair) in enumerate(zip(run.descs, run.offsets)):
        a = nu.arm(pics[i][3][sub]["picture"])
        assert np.array_equal(_luma_view(after, d, w, h), _luma_view(want, d, w, h)), ((w, h), i, a, "luma")
        for k, at in zip(("cb", "cr"), pair):
            assert np.array_equal(_chroma_view(after, at, run.cstride, w, h), _chroma_view(want, at, run.cstride, w, h)), ((w, h), i, a, k)
    assert np.array_equal(after, want)


def test_chain_detect_denoise_derive_statistics(hip_ctx):
    """one class-3_1 picture through the documented call order; the statistics are those of the reference's denoised planes"""
    torch = pytest.importorskip("torch")
    w, h, pics = nu.fixture_cases()[4]      # 200x136
    sub = 1
    luma, cb, cr, outs = pics[4]
    o = outs[sub]
    assert nu.arm(o["picture"]) == "whole_picture" and not np.array_equal(o["out_luma"], luma)
    run = _Run(torch, hip_ctx, [(luma, cb, cr)])
    run.detect(sub)
    run.denoise()
    ctx, n_sb = hip_ctx, run.n_sb
    shapes = {"y_mean": ((1, n_sb, 85), torch.uint8), "variance": ((1, n_sb, 85), torch.int16), "cb_mean": ((1, n_sb, 21), torch.uint8),
              "cr_mean": ((1, n_sb, 21), torch.uint8), "var_of_var": ((1, n_sb, 4), torch.int64), "homogeneous": ((1, n_sb), torch.uint8),
              "picture": ((1, 4), torch.int32), "histogram": ((1, 4, 4, 3, 256), torch.int32), "region_intensity": ((1, 4, 4, 3), torch.int32),
              "average_intensity": ((1, 3), torch.int32)}
    d = {k: torch.zeros(s, dtype=t, device="cuda:0") for k, (s, t) in shapes.items()}
    p = run.d_pool.data_ptr()
    ctx.pa_derive_planes_dev(p, run.descs)
    ctx.pa_block_stats_dev(p, run.descs, run.offsets, run.cstride, sub, d["y_mean"].data_ptr(), d["variance"].data_ptr(), d["cb_mean"].data_ptr(),
                           d["cr_mean"].data_ptr())
    ctx.pa_homogeneity_dev(d["variance"].data_ptr(), w, h, 1, d["var_of_var"].data_ptr(), d["homogeneous"].data_ptr(), d["picture"].data_ptr())
    ctx.pa_histograms_dev(p, run.descs, run.offsets, run.cstride, d["histogram"].data_ptr(), d["region_intensity"].data_ptr(), d["average_intensity"].data_ptr())
    ctx.synchronize()
    want = pu.all_stats(o["out_luma"], o["out_cb"], o["out_cr"], sub)
    for k in pu.OUTPUTS:
        assert np.array_equal(d[k][0].cpu().numpy().view(want[k].dtype).reshape(want[k].shape), want[k]), k


def test_caller_stream_without_synchronisation(hip_ctx):
    """detection and denoising of one fixture case on a caller's stream; the host waits on that stream alone"""
    torch = pytest.importorskip("torch")
    w, h, pics = nu.fixture_cases()[1]      # 136x72
    sub = 1
    run = _Run(torch, hip_ctx, [p[:3] for p in pics], s=torch.cuda.Stream())
    got = run.detect(sub)
    for i, (_, _, _, outs) in enumerate(pics):
        for k in nu.DETECT_OUTPUTS:
            assert np.array_equal(got[k][i], outs[sub][k]), (i, k)
        assert np.array_equal(got["denoised"][i][:, :w], outs[sub]["denoised"]), i
    after = run.denoise()
    assert np.array_equal(after, run.expected_pool([(p[3][sub]["out_luma"], p[3][sub]["out_cb"], p[3][sub]["out_cr"]) for p in pics]))


def test_refused_arguments(hip_ctx):
    """the library's error, and nothing launched: the outputs, d_denoised and the pool keep what they held"""
    torch = pytest.importorskip("torch")
    w, h, pics = nu.fixture_cases()[1]      # 136x72
    run = _Run(torch, hip_ctx, [pics[4][:3]])
    ctx, descs, offsets, cs, ds = hip_ctx, run.descs, run.offsets, run.cstride, run.dstride
    pool, den, var, flat, pic = (t.data_ptr() for t in (run.d_pool, run.d_den, run.d_var, run.d_flat, run.d_pic))

    def detect(pool_ptr=pool, d=descs, sub=1, den_ptr=den, stride=ds, outs=(var, flat, pic)):
        ctx.pa_noise_detect_dev(pool_ptr, d, sub, den_ptr, stride, *outs)

    def denoise(pool_ptr=pool, d=descs, offs=offsets, cstride=cs, den_ptr=den, stride=ds, flat_ptr=flat, pic_ptr=pic):
        ctx.pa_denoise_dev(pool_ptr, d, offs, cstride, den_ptr, stride, flat_ptr, pic_ptr)

    def changed(**kw):
        d = svtav1_hip.PaPictureDesc.from_buffer_copy(descs[0])
        for k, v in kw.items():
            setattr(d, k, v)
        return [d]

    refused = [lambda: detect(pool_ptr=None), lambda: detect(outs=(None, flat, pic)), lambda: detect(outs=(var, None, pic)), lambda: detect(outs=(var, flat, None)),
               lambda: detect(d=changed(width=132)), lambda: detect(d=changed(height=76)), lambda: detect(d=changed(width=56)), lambda: detect(d=changed(height=56)),
               lambda: detect(sub=2), lambda: detect(d=descs * 33), lambda: detect(stride=w - 8), lambda: detect(d=changed(full_stride=descs[0].full_stride - 4)),
               lambda: denoise(pool_ptr=None), lambda: denoise(den_ptr=None), lambda: denoise(flat_ptr=None), lambda: denoise(pic_ptr=None),
               lambda: denoise(d=changed(width=132)), lambda: denoise(d=changed(height=56)), lambda: denoise(d=descs * 33, offs=offsets * 33),
               lambda: denoise(stride=w - 8), lambda: denoise(offs=[[offsets[0][0] + 1, offsets[0][1]]]), lambda: denoise(offs=[[offsets[0][0], offsets[0][1] - 1]]),
               lambda: denoise(cstride=cs + 1), lambda: denoise(d=changed(full_stride=descs[0].full_stride - 4))]
    for call in refused:
        with pytest.raises(svtav1_hip.SvtHipError, match="80001005"):
            call()
    ctx.synchronize()
    assert (run.d_den.cpu().numpy() == FILL8).all() and (run.d_flat.cpu().numpy() == FILL8).all()
    assert (run.d_var.cpu().numpy() == FILL64).all() and (run.d_pic.cpu().numpy() == FILL32).all()
    assert np.array_equal(run.d_pool.cpu().numpy(), run.pool)
