"""GPU: the picture-analysis statistics entries (svthip_pa_block_stats_dev, svthip_pa_homogeneity_dev, svthip_pa_histograms_dev) through the
C ABI, bit-exact against the reference's fixture (tests/golden/pa_stats.npz) and the restatement (tests/pa_stats_util.py).  The pool is
uploaded with picture interiors only and svthip_pa_derive_planes_dev builds the borders and the 1/16 planes on the device: the real call
sequence, and the proof of the incomplete SBs' luma reads.  The chroma planes lie at offsets and a stride that are even and not multiples
of 4, so their rows start on and off dword boundaries."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import pa_stats_util as pu  # noqa: E402
import svtav1_hip  # noqa: E402
from svtav1_hip import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def _pool(planes):
    """planes: [(luma, cb, cr)] of one size -> (pool with interiors only, descriptors, chroma offsets, chroma stride)"""
    pics = [synth.PaPicture(luma) for luma, _, _ in planes]
    laid_out, descs = svtav1_hip.build_picture_pool(pics)
    h, w = planes[0][0].shape
    cstride = w // 2 + 2
    luma_bytes = laid_out.size + 2                       # chroma starts 2 past a multiple of 4
    pool = np.full(luma_bytes + len(planes) * 2 * cstride * (h // 2) + 256, 0xEE, np.uint8)
    offsets, at = [], luma_bytes
    for (luma, cb, cr), d in zip(planes, descs):
        fs = d.full_stride
        full = pool[d.full_offset:d.full_offset + fs * (h + 136)].reshape(h + 136, fs)
        full[68:68 + h, 68:68 + w] = luma
        pair = []
        for c in (cb, cr):
            pool[at:at + cstride * (h // 2)].reshape(h // 2, cstride)[:, :w // 2] = c
            pair.append(at)
            at += cstride * (h // 2)
        offsets.append(pair)
    return pool, descs, offsets, cstride


def _run(torch, ctx, planes, sub, entries=(1, 2, 3), s=None):
    """the three entries over the pictures of one launch -> {output: [n] + shape}.  s: a torch stream that every call is given; the
    outputs are then read back behind the calls on that stream and the context is not synchronised"""
    pool, descs, offsets, cstride = _pool(planes)
    h, w = planes[0][0].shape
    n, n_sb = len(planes), pu.sb_grid(w, h)[0] * pu.sb_grid(w, h)[1]
    d_pool = torch.from_numpy(pool).to("cuda:0")
    shapes = {"y_mean": ((n, n_sb, 85), torch.uint8), "variance": ((n, n_sb, 85), torch.int16), "cb_mean": ((n, n_sb, 21), torch.uint8),
              "cr_mean": ((n, n_sb, 21), torch.uint8), "var_of_var": ((n, n_sb, 4), torch.int64), "homogeneous": ((n, n_sb), torch.uint8),
              "picture": ((n, 4), torch.int32), "histogram": ((n, 4, 4, 3, 256), torch.int32), "region_intensity": ((n, 4, 4, 3), torch.int32),
              "average_intensity": ((n, 3), torch.int32)}
    d = {k: torch.full(s, 0xAA if t == torch.uint8 else -1431655766 if t == torch.int32 else -21846 if t == torch.int16 else -6148914691236517206,
                       dtype=t, device="cuda:0") for k, (s, t) in shapes.items()}
    stream = s.cuda_stream if s is not None else None
    if s is None:
        torch.cuda.synchronize()
    else:
        s.wait_stream(torch.cuda.current_stream())   # stream order behind the upload and the fills, not a host wait
    ctx.pa_derive_planes_dev(d_pool.data_ptr(), descs, stream=stream)
    if 1 in entries:
        ctx.pa_block_stats_dev(d_pool.data_ptr(), descs, offsets, cstride, sub, d["y_mean"].data_ptr(), d["variance"].data_ptr(), d["cb_mean"].data_ptr(),
                               d["cr_mean"].data_ptr(), stream=stream)
    if 2 in entries:
        ctx.pa_homogeneity_dev(d["variance"].data_ptr(), w, h, n, d["var_of_var"].data_ptr(), d["homogeneous"].data_ptr(), d["picture"].data_ptr(),
                               stream=stream)
    if 3 in entries:
        ctx.pa_histograms_dev(d_pool.data_ptr(), descs, offsets, cstride, d["histogram"].data_ptr(), d["region_intensity"].data_ptr(),
                              d["average_intensity"].data_ptr(), stream=stream)
    unsigned = {torch.uint8: np.uint8, torch.int16: np.uint16, torch.int32: np.uint32, torch.int64: np.uint64}
    if s is None:
        ctx.synchronize()
        return {k: t.cpu().numpy().view(unsigned[shapes[k][1]]) for k, t in d.items()}
    with torch.cuda.stream(s):
        host = {k: t.to("cpu") for k, t in d.items()}   # enqueued on s behind the entries
    return {k: t.numpy().view(unsigned[shapes[k][1]]) for k, t in host.items()}


@pytest.mark.parametrize("sub", (0, 1))
@pytest.mark.parametrize("c", range(len(pu.CASES)))
def test_entries_match_fixture(hip_ctx, c, sub):
    """every picture of a case in one launch, through the three entries"""
    torch = pytest.importorskip("torch")
    w, h, pics = pu.fixture_cases()[c]
    got = _run(torch, hip_ctx, [p[:3] for p in pics], sub)
    complete = pu.complete_sbs(w, h)
    for i, (luma, cb, cr, outs) in enumerate(pics):
        mine = pu.all_stats(luma, cb, cr, sub)
        for k in pu.OUTPUTS:
            assert np.array_equal(got[k][i], outs[sub][k]) and np.array_equal(mine[k], outs[sub][k]), ((w, h), i, sub, k)
        # the outputs were filled with 0xAA: the chroma means of incomplete SBs were written, as zeros
        assert (got["cb_mean"][i][~complete] == 0).all() and (got["cr_mean"][i][~complete] == 0).all()


def test_batch_of_three_equals_three_single_launches(hip_ctx):
    torch = pytest.importorskip("torch")
    w, h, pics = pu.fixture_cases()[3]      # 200x136
    three = [pics[i][:3] for i in (1, 4, 7)]   # noise, checkerboard, odd rows unlike even rows
    batch = _run(torch, hip_ctx, three, 1)
    for i, planes in enumerate(three):
        single = _run(torch, hip_ctx, [planes], 1)
        for k in pu.OUTPUTS:
            assert np.array_equal(batch[k][i], single[k][0]), (i, k)


def test_caller_stream_without_synchronisation(hip_ctx):
    """one fixture picture through svthip_pa_derive_planes_dev and the three entries on a caller's stream, svthip_pa_histograms_dev with
    its region sums in context scratch among them; twice, so that the second run finds the scratch as the first left it"""
    torch = pytest.importorskip("torch")
    w, h, pics = pu.fixture_cases()[3]      # 200x136
    luma, cb, cr, outs = pics[1]
    for _ in range(2):
        got = _run(torch, hip_ctx, [(luma, cb, cr)], 1, s=torch.cuda.Stream())
        for k in pu.OUTPUTS:
            assert np.array_equal(got[k][0], outs[1][k]), k


def test_refused_arguments(hip_ctx):
    """the library's error, and nothing launched: the outputs keep their fill"""
    torch = pytest.importorskip("torch")
    w, h, pics = pu.fixture_cases()[1]      # 136x72
    planes = [pics[1][:3]]
    pool, descs, offsets, cstride = _pool(planes)
    d_pool = torch.from_numpy(pool).to("cuda:0")
    out = torch.full((1 << 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
    o = [out.data_ptr() + 8192 * k for k in range(4)]
    ctx = hip_ctx
    ctx.pa_derive_planes_dev(d_pool.data_ptr(), descs)

    def block(pool_ptr=d_pool.data_ptr(), ds=descs, offs=offsets, cs=cstride, sub=1, outs=o):
        ctx.pa_block_stats_dev(pool_ptr, ds, offs, cs, sub, *outs)

    def hist(ds=descs, offs=offsets, cs=cstride, outs=o[:3]):
        ctx.pa_histograms_dev(d_pool.data_ptr(), ds, offs, cs, *outs)

    def changed(**kw):
        d = svtav1_hip.PaPictureDesc.from_buffer_copy(descs[0])
        for k, v in kw.items():
            setattr(d, k, v)
        return [d]

    refused = [lambda: block(pool_ptr=None), lambda: block(outs=[o[0], None, o[2], o[3]]), lambda: block(ds=changed(width=132)),
               lambda: block(ds=changed(height=76)), lambda: block(ds=changed(width=8)), lambda: block(offs=[[offsets[0][0] + 1, offsets[0][1]]]),
               lambda: block(offs=[[offsets[0][0], -2]]), lambda: block(cs=cstride + 1), lambda: block(sub=2), lambda: block(ds=descs * 33, offs=offsets * 33),
               lambda: block(ds=changed(full_stride=descs[0].full_stride - 4)),
               lambda: hist(outs=[o[0], o[1], None]), lambda: hist(ds=changed(height=8)), lambda: hist(offs=[[offsets[0][0], offsets[0][1] + 1]]),
               lambda: hist(ds=descs * 33, offs=offsets * 33), lambda: hist(ds=changed(sixteenth_stride=(w >> 2) + 30)),
               lambda: ctx.pa_homogeneity_dev(None, 136, 72, 1, o[1], o[2], o[3]), lambda: ctx.pa_homogeneity_dev(o[0], 56, 72, 1, o[1], o[2], o[3]),
               lambda: ctx.pa_homogeneity_dev(o[0], 136, 60, 1, o[1], o[2], o[3]), lambda: ctx.pa_homogeneity_dev(o[0], 136, 72, 33, o[1], o[2], o[3])]
    for k, call in enumerate(refused):
        with pytest.raises(svtav1_hip.SvtHipError, match="80001005"):
            call()
    ctx.synchronize()
    assert (out.cpu().numpy() == 0xAA).all()
