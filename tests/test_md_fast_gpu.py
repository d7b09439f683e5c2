"""GPU: mode decision's fast loop (svthip_md_fast_cost_batch_dev, svthip_md_fast_pick_batch_dev) through the C ABI, bit-exact against the
reference's fixture (tests/golden/md_fast.npz) and the restatement (tests/md_fast_util.py).  Every plane sits inside a larger buffer of
garbage, once with a stride and a base that are multiples of 4 (every quad one dword load) and once each 1, 2 and 3 bytes into its buffer at
an odd stride (the byte path); the samples right around every prediction tile are 0 and 255, so a sum that strays changes.  The chain
test runs the inter prediction entry, the cost entry and the pick entry on one stream with nothing in between."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import md_fast_util as mu  # noqa: E402
import svtav1_hip  # noqa: E402

pytestmark = pytest.mark.gpu

BAD = "80001005"
LAYOUTS = (0, 1, 2, 3)   # bytes between a plane's buffer and its sample (0, 0); 0: strides multiples of 4, else odd strides
BAD_GROUPS = [(0, 0, 3, 13), (0, 114, 3, 13), (0, 3, 3, 0), (0, 3, 3, 14), (0, 3, 0, 13), (0, 3, 13, 13), (None, 3, 3, 13)]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


class _Planes:
    """Y, Cb, Cr inside garbage on the device; Cb and Cr share a stride"""

    def __init__(self, torch, planes, shift):
        self.keep = []
        ptrs, strides = [], []
        for k, p in enumerate(planes):
            h, w = p.shape
            wide = planes[1].shape[1] if k else w
            stride = (wide + 11) // 4 * 4 if shift == 0 else (wide + 8) | 1
            buf = np.full((h + 2) * stride + 8, 0x3C, np.uint8)
            buf[1::3] = 0xC3
            rows = buf[stride + shift:stride + shift + h * stride].reshape(h, stride)
            rows[:, :w] = p
            t = _dev(torch, buf)
            self.keep.append(t)
            ptrs.append(t.data_ptr() + stride + shift)
            strides.append(stride)
        assert strides[1] == strides[2]
        self.arg = svtav1_hip.InterPlanes()
        self.arg.y, self.arg.cb, self.arg.cr = ptrs
        self.arg.y_stride, self.arg.c_stride = strides[0], strides[1]


def _run_cost(torch, ctx, src, pool, desc, w, h, stream=None):
    d_desc = _dev(torch, desc)
    d_result = torch.full((len(desc) * 16 + 16,), 0x77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.md_fast_cost_batch_dev(src.arg, pool.arg, d_desc.data_ptr(), len(desc), w, h, d_result.data_ptr(), stream=stream)
    ctx.synchronize()
    if stream is not None:
        torch.cuda.synchronize()
    raw = d_result.cpu().numpy()
    assert (raw[len(desc) * 16:] == 0x77).all(), "wrote behind the last result"
    return raw[:len(desc) * 16].view(mu.RESULT_DTYPE)


@pytest.fixture(scope="module")
def source():
    return mu.source_planes()


@pytest.mark.parametrize("z", range(len(mu.SIZES)))
def test_every_size_bit_exact(hip_ctx, source, z):
    torch = pytest.importorskip("torch")
    w, h = mu.SIZES[z]
    pool = mu.pool_planes(z, source)
    fx = mu.fixture()
    batches = {n: mu.descriptors(z, n, variant=n) for n in (6, 1, 5, 67)}
    batches[13] = mu.descriptors(z, 13)
    want = {n: mu.fast_cost(source, pool, d, w, h) for n, d in batches.items()}
    assert np.array_equal(want[13], np.ascontiguousarray(fx[f"result_z{z}"]).view(mu.RESULT_DTYPE).reshape(-1)), "the restatement left the fixture"
    assert {0, 1} == set(batches[6]["has_uv"].tolist()) and len(set(batches[67]["flags"].tolist())) == len(mu.flag_sets())
    for shift in LAYOUTS:
        d_src, d_pool = _Planes(torch, source, shift), _Planes(torch, pool, shift)
        for n in ((6, 13, 1, 5, 67) if shift in (0, 3) else (6, 13)):
            got = _run_cost(torch, hip_ctx, d_src, d_pool, batches[n], w, h)
            bad = np.flatnonzero(got != want[n])
            assert bad.size == 0, ((w, h), shift, n, bad[:6], got[bad[:3]], want[n][bad[:3]])
    # n_cand == 0: nothing is looked at
    hip_ctx.md_fast_cost_batch_dev(None, None, None, 0, w, h, None)


def _pick_arrays():
    result, desc, groups = mu.pick_inputs()
    bad = np.array([(len(result) - 2 if f is None else f, c, t, b) for f, c, t, b in BAD_GROUPS], mu.GROUP_DTYPE)
    return result, desc, groups, bad


def _run_pick(torch, ctx, result, desc, groups, stream=None):
    d_result, d_desc, d_groups = _dev(torch, result), _dev(torch, desc), _dev(torch, groups)
    d_pick = torch.full((len(groups) * 32 + 32,), 0x77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.md_fast_pick_batch_dev(d_result.data_ptr(), d_desc.data_ptr(), len(result), d_groups.data_ptr(), len(groups), d_pick.data_ptr(), stream=stream)
    ctx.synchronize()
    if stream is not None:
        torch.cuda.synchronize()
    raw = d_pick.cpu().numpy()
    assert (raw[len(groups) * 32:] == 0x77).all(), "wrote behind the last pick"
    return raw[:len(groups) * 32].view(mu.PICK_DTYPE)


def test_pick_matches_reference_fixture(hip_ctx):
    """1 candidate, count ==, < and > buffer_total_count, 113 candidates over 13 buffers, ties that tell > from >= in the walk and in
    PreModeDecision, every cost ~0, intra and inter interleaved: md_fast_util.pick_cases"""
    torch = pytest.importorskip("torch")
    result, desc, groups, _ = _pick_arrays()
    hip_ctx.inter_pred_refused()
    got = _run_pick(torch, hip_ctx, result, desc, groups)
    want = np.ascontiguousarray(mu.fixture()["pick"]).view(mu.PICK_DTYPE).reshape(-1)
    for name, g, w_ in zip(mu.fixture()["pick_names"], got, want):
        assert g == w_, (name, g, w_)
    assert np.array_equal(got, mu.pick(result, desc, groups)[0])
    assert hip_ctx.inter_pred_refused() == 0
    # more than one workgroup, the last one partial
    many = np.tile(groups, 7)[:150]
    assert np.array_equal(_run_pick(torch, hip_ctx, result, desc, many), np.tile(want, 7)[:150])
    assert hip_ctx.inter_pred_refused() == 0


def test_pick_refuses_groups_on_the_device(hip_ctx):
    torch = pytest.importorskip("torch")
    result, desc, groups, bad = _pick_arrays()
    hip_ctx.inter_pred_refused()
    mixed = np.concatenate([groups[:3], bad, groups[3:]])
    got = _run_pick(torch, hip_ctx, result, desc, mixed)
    want, refused = mu.pick(result, desc, mixed)
    assert refused == len(bad) == 7 and np.array_equal(got, want)
    assert (got["full_count"][3:3 + len(bad)] == 0).all() and (got["best"][3:3 + len(bad)] == 0xFF).all()
    with pytest.raises(svtav1_hip.SvtHipError, match=rf"{BAD}: 7 PU\(s\) or unit\(s\) refused.*fast-loop group out of range \(svthip_md_fast_pick_batch_dev\)"):
        hip_ctx.inter_pred_refused()
    assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("size", [(8, 8), (16, 8)])
def test_prediction_cost_and_pick_chain_on_one_stream(hip_ctx, size):
    """svthip_av1_inter_pred_batch_dev writes the tiles, the cost entry measures them, the pick entry walks the costs: three calls on one
    stream, the host waits only at the end"""
    torch = pytest.importorskip("torch")
    import inter_pred_util as ipu
    bw, bh = size
    rng = np.random.default_rng(bw * 100 + bh)
    pic_w, pic_h = 128, 64
    refs = [ipu.random_picture(rng, pic_w, pic_h, ipu.border_for(bw, bh), 8, kind) for kind in ("noise", "smooth")]
    n = (pic_w // bw) * (pic_h // bh) - 3
    pu = ipu.random_descs(rng, n, bw, bh, pic_w, pic_h, clamp_frac=0.1)
    cur = ipu.random_picture(rng, pic_w, pic_h, 0, 8, "smooth")
    blank = lambda: ipu.Picture(np.full((pic_h, pic_w), 0x55, np.uint8), *(np.full((pic_h // 2, pic_w // 2), 0x55, np.uint8) for _ in range(2)), 0)  # noqa: E731
    desc = np.zeros(n, mu.DESC_DTYPE)
    desc["src_x"], desc["src_y"], desc["pred_x"], desc["pred_y"] = pu["pu_origin_x"], pu["pu_origin_y"], pu["dst_origin_x"], pu["dst_origin_y"]
    desc["rate"], desc["merge_rate"], desc["lambda_"] = rng.integers(100, 5000, n), mu.NO_MERGE, 2000
    desc["has_uv"], desc["flags"] = pu["has_uv"], np.where(rng.random(n) < 0.5, mu.TYPE_INTER, 0)
    groups = np.array([(g * 6, min(6, n - g * 6), 3, 13) for g in range((n + 5) // 6)], mu.GROUP_DTYPE)
    # numpy
    pred = blank()
    assert ipu.predict(refs[0], refs[1], pred, pu, bw, bh, 8) == 0
    want = mu.fast_cost((cur.y, cur.cb, cur.cr), (pred.y, pred.cb, pred.cr), desc, bw, bh)
    want_pick, refused = mu.pick(want, desc, groups)
    assert refused == 0 and len(set(want["cost"].tolist())) > n // 2
    # device
    d0, d1, dp, dc = ipu.to_device(refs[0]), ipu.to_device(refs[1]), ipu.to_device(blank()), ipu.to_device(cur)
    d_pu, d_desc, d_groups = _dev(torch, pu), _dev(torch, desc), _dev(torch, groups)
    d_result = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    d_pick = torch.zeros(len(groups) * 32, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    p_pred, p_cur = ipu.planes_of(dp, pred), ipu.planes_of(dc, cur)
    hip_ctx.av1_inter_pred_batch_dev(ipu.planes_of(d0, refs[0]), ipu.planes_of(d1, refs[1]), p_pred, d_pu.data_ptr(), n, bw, bh, stream=s.cuda_stream)
    hip_ctx.md_fast_cost_batch_dev(p_cur, p_pred, d_desc.data_ptr(), n, bw, bh, d_result.data_ptr(), stream=s.cuda_stream)
    hip_ctx.md_fast_pick_batch_dev(d_result.data_ptr(), d_desc.data_ptr(), n, d_groups.data_ptr(), len(groups), d_pick.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_result.cpu().numpy().view(mu.RESULT_DTYPE), want)
    assert np.array_equal(d_pick.cpu().numpy().view(mu.PICK_DTYPE), want_pick)
    assert hip_ctx.inter_pred_refused() == 0


def test_context_reuse_and_refusals(source):
    torch = pytest.importorskip("torch")
    ctx = svtav1_hip.Context(0)
    try:
        # two sizes on one context, the second on another stream
        s = torch.cuda.Stream()
        for z, stream in ((3, None), (12, s.cuda_stream), (0, None)):
            w, h = mu.SIZES[z]
            pool = mu.pool_planes(z, source)
            desc = mu.descriptors(z, 6)
            got = _run_cost(torch, ctx, _Planes(torch, source, 0), _Planes(torch, pool, 0), desc, w, h, stream=stream)
            assert np.array_equal(got, mu.fast_cost(source, pool, desc, w, h)), (w, h)

        w, h = 8, 8
        d_src, d_pool = _Planes(torch, source, 0), _Planes(torch, mu.pool_planes(3, source), 0)
        desc = mu.descriptors(3, 6)
        d_desc = _dev(torch, np.concatenate([desc, desc]))
        d_result = torch.zeros(16 * 16, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ok = dict(src=d_src.arg, pred=d_pool.arg, d_desc=d_desc.data_ptr(), n_cand=6, bwidth=w, bheight=h, d_result=d_result.data_ptr())

        def refused(words, call, **change):
            with pytest.raises(svtav1_hip.SvtHipError, match=f"{BAD}.*{words}"):
                call(**{**(ok if call == ctx.md_fast_cost_batch_dev else ok_pick), **change})

        cost = ctx.md_fast_cost_batch_dev
        for bw, bh in ((8, 64), (12, 8), (0, 0), (256, 128), (64, 8)):
            refused("not an AV1 block size", cost, bwidth=bw, bheight=bh)
        refused("not an AV1 block size", cost, bwidth=8, bheight=64, n_cand=0)    # the size is checked before the count
        for k in ("src", "pred", "d_desc", "d_result"):
            refused("null pointer", cost, **{k: None})
        for which in ("src", "pred"):
            for plane in ("y", "cb", "cr"):
                p = svtav1_hip.InterPlanes()
                for f in ("y", "cb", "cr", "y_stride", "c_stride"):
                    setattr(p, f, getattr(ok[which], f))
                setattr(p, plane, None)
                refused("null plane pointer", cost, **{which: p})
        refused("descriptor array must be 16-byte aligned", cost, d_desc=d_desc.data_ptr() + 8)
        refused("result array must be 16-byte aligned", cost, d_result=d_result.data_ptr() + 8)
        cost(None, None, None, 0, w, h, None)                                       # n_cand == 0 returns OK
        cost(**ok)

        result, p_desc, groups, _ = _pick_arrays()
        d_r, d_d, d_g = _dev(torch, result), _dev(torch, p_desc), _dev(torch, np.concatenate([groups, groups]))
        d_pick = torch.zeros((len(groups) + 1) * 32, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ok_pick = dict(d_result=d_r.data_ptr(), d_desc=d_d.data_ptr(), n_cand=len(result), d_group=d_g.data_ptr(), n_groups=len(groups), d_pick=d_pick.data_ptr())
        pick = ctx.md_fast_pick_batch_dev
        for k in ("d_result", "d_desc", "d_group", "d_pick"):
            refused("null pointer", pick, **{k: None})
        for k in ("d_result", "d_desc", "d_pick"):
            refused("must be 16-byte aligned", pick, **{k: ok_pick[k] + 8})
        refused("group array must be 8-byte aligned", pick, d_group=ok_pick["d_group"] + 4)
        pick(None, None, 0, None, 0, None)                                          # n_groups == 0 returns OK
        pick(**ok_pick)
        ctx.synchronize()
        assert ctx.inter_pred_refused() == 0
        assert np.array_equal(d_pick.cpu().numpy()[:len(groups) * 32].view(mu.PICK_DTYPE), mu.pick(result, p_desc, groups)[0])
    finally:
        ctx.close()
