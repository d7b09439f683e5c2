"""GPU: svthip_av1_[highbd_]warped_pred_batch_dev (warped-motion prediction of whole PUs: Y / Cb / Cr, warped or translational chroma)
bit-exact against the reference's fixture (tests/golden/warp.npz), against the numpy restatement on random batches of every size, against
the translational whole-PU entry for the chroma of blocks below 16x16; picture sizes that are not multiples of 8 and 3840 x 2160; the
caller-stream contract, every refusal on the host and on the device, and call sequences on one context."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import inter_pred_util as ipu  # noqa: E402
import svtav1_hip  # noqa: E402
import warp_util as wu  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "warp.npz")


def _compare(got, want, tag, planes=("y", "cb", "cr")):
    for p in planes:
        g, w = getattr(got, p), getattr(want, p)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (tag, p, len(bad), bad[:4], g[tuple(bad[0])], w[tuple(bad[0])])


def _blank(pic_w, pic_h, bd):
    dt = np.uint8 if bd == 8 else np.uint16
    f = 0x55 if bd == 8 else 0x155
    return ipu.Picture(np.full((pic_h, pic_w), f, dt), np.full((pic_h // 2, pic_w // 2), f, dt), np.full((pic_h // 2, pic_w // 2), f, dt), 0)


@pytest.mark.parametrize("bd", [8, 10])
def test_fixture_bit_exact(hip_ctx, bd):
    pytest.importorskip("torch")
    from make_golden_warp import PIC, reference_picture
    g = dict(np.load(GOLDEN))
    ref = reference_picture(bd)
    n_cases = 0
    for i in range(len(g["case_bw"])):
        if int(g["case_bd"][i]) != bd:
            continue
        bw, bh = int(g["case_bw"][i]), int(g["case_bh"][i])
        s, n = int(g["case_start"][i]), int(g["case_count"][i])
        desc = g["desc"][s:s + n].view(svtav1_hip.WARP_PU_DESC_DTYPE)
        got, _ = wu.run_device(hip_ctx, ref, _blank(PIC, PIC, bd), desc, bw, bh, bd, PIC, PIC)
        r = int(g["case_pred"][i])
        want = ipu.Picture(g[f"pred_y_{bd}"][r], g[f"pred_cb_{bd}"][r], g[f"pred_cr_{bd}"][r], 0)
        _compare(got, want, (i, bw, bh, bd))
        n_cases += 1
    assert n_cases >= 17
    assert hip_ctx.inter_pred_refused() == 0


def _random_batch(size, bd, seed, pic_w=512, pic_h=256, n_max=1500, positions=None):
    bw, bh = size
    rng = np.random.default_rng(seed)
    ref = ipu.random_picture(rng, pic_w, pic_h, ipu.border_for(bw, bh), bd, "smooth" if seed & 1 else "noise")
    n = min((pic_w // bw) * (pic_h // bh), n_max) - 3   # leaves a partial last workgroup of the warp kernel (16 blocks per group)
    desc = wu.random_descs(rng, n, bw, bh, pic_w, pic_h, edge_frac=0.3, clamp_frac=0.2, positions=positions)
    return ref, desc


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", svtav1_hip.WARP_BLOCK_SIZES_WH)
def test_random_batches_match_restatement(hip_ctx, size, bd):
    pytest.importorskip("torch")
    bw, bh = size
    ref, desc = _random_batch(size, bd, bw * 1000 + bh * 10 + bd)
    per_pu = (bw // 8) * (bh // 8) + (2 * (bw // 16) * (bh // 16) if bw >= 16 and bh >= 16 else 0)
    assert (len(desc) * per_pu) % 16 != 0 or per_pu % 16 == 0   # a partial last workgroup wherever the size allows one
    stats = wu.new_stats()
    want = _blank(512, 256, bd)
    assert wu.predict(ref, want, desc, bw, bh, bd, 512, 256, stats) == 0
    assert {e for _, e in stats["edges"]} == {"left", "right", "top", "bottom"} or len(desc) < 100
    got, _ = wu.run_device(hip_ctx, ref, _blank(512, 256, bd), desc, bw, bh, bd, 512, 256)
    _compare(got, want, (size, bd))
    assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", [s for s in svtav1_hip.WARP_BLOCK_SIZES_WH if min(s) == 8])
def test_translational_chroma_equals_inter_pred_entry(hip_ctx, size, bd):
    """Cb and Cr of blocks below 16x16 against svthip_av1_inter_pred_batch_dev given the same vector, edges, interp_filters = 0 and
    pred_direction = 0 (device against device)"""
    pytest.importorskip("torch")
    bw, bh = size
    ref, desc = _random_batch(size, bd, 77 * bw + bh + bd, n_max=600)
    desc["has_uv"] = 1
    tr = np.zeros(len(desc), svtav1_hip.INTER_PU_DESC_DTYPE)
    for k in ("pu_origin_x", "pu_origin_y", "dst_origin_x", "dst_origin_y", "mb_to_left_edge", "mb_to_right_edge", "mb_to_top_edge", "mb_to_bottom_edge",
              "has_uv"):
        tr[k] = desc[k]
    tr["mv"][:, 0, :] = desc["mv"]
    got, _ = wu.run_device(hip_ctx, ref, _blank(512, 256, bd), desc, bw, bh, bd, 512, 256)
    want, _ = ipu.run_device(hip_ctx, ref, ref, _blank(512, 256, bd), tr, bw, bh, bd)
    _compare(got, want, (size, bd), planes=("cb", "cr"))
    assert not np.array_equal(got.cb, _blank(512, 256, bd).cb)
    assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_odd_picture_size_and_4k_corner(hip_ctx, bd):
    pytest.importorskip("torch")
    for size in ((8, 8), (16, 16), (64, 32)):
        bw, bh = size
        ref, desc = _random_batch(size, bd, 5000 + bw + bd, pic_w=500, pic_h=250, n_max=300)
        want = _blank(500, 250, bd)
        assert wu.predict(ref, want, desc, bw, bh, bd, 500, 250) == 0
        got, _ = wu.run_device(hip_ctx, ref, _blank(500, 250, bd), desc, bw, bh, bd, 500, 250)
        _compare(got, want, ("500x250", size, bd))
    W, H = 3840, 2160
    for size in ((8, 16), (32, 32), (128, 128)):
        bw, bh = size
        pos = [(W - bw * (1 + i % 4), H - bh * (1 + i // 4)) for i in range(11)]
        rng = np.random.default_rng(6000 + bw + bd)
        ref = ipu.random_picture(rng, W, H, ipu.border_for(bw, bh), bd, "noise")
        desc = wu.random_descs(rng, len(pos), bw, bh, W, H, edge_frac=0.4, clamp_frac=0.3, positions=pos)
        want = _blank(W, H, bd)
        assert wu.predict(ref, want, desc, bw, bh, bd, W, H) == 0
        got, _ = wu.run_device(hip_ctx, ref, _blank(W, H, bd), desc, bw, bh, bd, W, H)
        _compare(got, want, ("4K", size, bd))
    assert hip_ctx.inter_pred_refused() == 0


def test_caller_stream_without_synchronisation(hip_ctx):
    torch = pytest.importorskip("torch")
    for bd, size in ((8, (8, 8)), (10, (16, 8)), (8, (64, 64)), (10, (32, 32))):
        bw, bh = size
        ref, desc = _random_batch(size, bd, 900 + bd + bw)
        want = _blank(512, 256, bd)
        wu.predict(ref, want, desc, bw, bh, bd, 512, 256)
        s = torch.cuda.Stream()
        d0, dp = ipu.to_device(ref), ipu.to_device(_blank(512, 256, bd))
        d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        s.wait_stream(torch.cuda.current_stream())   # stream order, not a host wait
        args = (ipu.planes_of(d0, ref), ipu.planes_of(dp, want), 512, 256, d_desc.data_ptr(), len(desc), bw, bh)
        with torch.cuda.stream(s):
            if bd == 8:
                hip_ctx.av1_warped_pred_batch_dev(*args, stream=s.cuda_stream)
            else:
                hip_ctx.av1_highbd_warped_pred_batch_dev(*args, bit_depth=10, stream=s.cuda_stream)
            host = {p: dp[p].to("cpu") for p in ("y", "cb", "cr")}   # enqueued on s behind the prediction
        got = ipu.Picture(host["y"].numpy(), host["cb"].numpy(), host["cr"].numpy(), 0)
        _compare(got, want, ("stream", size, bd))
    assert hip_ctx.inter_pred_refused() == 0


def test_refusals(hip_ctx):
    torch = pytest.importorskip("torch")
    bd = 8
    E = svtav1_hip.SvtHipError
    for (bw, bh) in ((8, 8), (16, 16)):
        ref, desc = _random_batch((bw, bh), bd, 4242 + bw, n_max=400)
        d0, dp = ipu.to_device(ref), ipu.to_device(_blank(512, 256, bd))
        p0, pp = ipu.planes_of(d0, ref), ipu.planes_of(dp, _blank(512, 256, bd))
        d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
        n = len(desc)
        for bad_size in ((12, 12), (4, 4), (4, 8), (8, 4), (4, 16), (16, 4), (8, 64)):
            with pytest.raises(E, match="block size"):
                hip_ctx.av1_warped_pred_batch_dev(p0, pp, 512, 256, d_desc.data_ptr(), n, *bad_size)
        with pytest.raises(E, match="null"):
            hip_ctx.av1_warped_pred_batch_dev(None, pp, 512, 256, d_desc.data_ptr(), n, bw, bh)
        with pytest.raises(E, match="null"):
            hip_ctx.av1_warped_pred_batch_dev(p0, None, 512, 256, d_desc.data_ptr(), n, bw, bh)
        with pytest.raises(E, match="null"):
            hip_ctx.av1_warped_pred_batch_dev(p0, pp, 512, 256, None, n, bw, bh)
        hole = svtav1_hip.InterPlanes(p0.y, None, p0.cr, p0.y_stride, p0.c_stride)
        with pytest.raises(E, match="null"):
            hip_ctx.av1_warped_pred_batch_dev(hole, pp, 512, 256, d_desc.data_ptr(), n, bw, bh)
        with pytest.raises(E, match="16-byte"):
            hip_ctx.av1_warped_pred_batch_dev(p0, pp, 512, 256, buf.data_ptr() + 4, n, bw, bh)
        for (w, h) in ((0, 256), (512, 0), (65536, 256), (512, 70000)):
            with pytest.raises(E, match="pic_width"):
                hip_ctx.av1_warped_pred_batch_dev(p0, pp, w, h, d_desc.data_ptr(), n, bw, bh)
        with pytest.raises(E, match="bit_depth"):
            hip_ctx.av1_highbd_warped_pred_batch_dev(p0, pp, 512, 256, d_desc.data_ptr(), n, bw, bh, bit_depth=12)
        with pytest.raises(E, match="bit_depth"):
            hip_ctx.av1_highbd_warped_pred_batch_dev(p0, pp, 512, 256, d_desc.data_ptr(), n, bw, bh, bit_depth=8)
        odd = svtav1_hip.InterPlanes(p0.y, p0.cb + 1, p0.cr, p0.y_stride, p0.c_stride)          # 16-bit planes are 2-byte aligned
        with pytest.raises(E, match="2-byte"):
            hip_ctx.av1_highbd_warped_pred_batch_dev(odd, pp, 512, 256, d_desc.data_ptr(), n, bw, bh, bit_depth=10)
        hip_ctx.av1_warped_pred_batch_dev(None, None, 512, 256, None, 0, bw, bh)               # n_pu == 0: OK
        assert hip_ctx.inter_pred_refused() == 0                                               # nothing refused so far

        # models the reference's validity tests reject and model types warp_plane does not take: refused on the device, nothing written
        # for them (their chroma included), their neighbours correct, counted
        bad = desc.copy()
        bad["has_uv"][:12] = 1
        bad[1]["alpha"] = 16384                       # 4 |alpha| >= 65536
        bad[3]["beta"] = -9408                        # 7 |beta| >= 65536
        bad[4]["gamma"], bad[4]["delta"] = 8192, -8192
        bad[6]["wmmat"][2] = 0                        # is_affine_valid
        bad[7]["wmmat"][2] = -65536
        bad[9]["wmtype"] = 1                          # TRANSLATION
        bad[10]["wmtype"] = 4
        bad[n - 1]["delta"] = 16384
        n_bad = 8
        want = _blank(512, 256, bd)
        assert wu.predict(ref, want, bad, bw, bh, bd, 512, 256) == n_bad
        got, _ = wu.run_device(hip_ctx, ref, _blank(512, 256, bd), bad, bw, bh, bd, 512, 256)
        _compare(got, want, ("refused", bw, bh))
        with pytest.raises(E, match=f"{n_bad} PU"):
            hip_ctx.inter_pred_refused()
        assert hip_ctx.inter_pred_refused() == 0                                               # the count was cleared


def test_sequences_on_one_context():
    """small picture -> svthip_reserve for a large one -> small again, warped and translational calls interleaved: results unchanged"""
    pytest.importorskip("torch")
    ctx = svtav1_hip.Context(0)
    try:
        warp = {}
        for size, bd in (((8, 8), 8), ((32, 32), 8), ((16, 8), 10), ((64, 64), 10)):
            ref, desc = _random_batch(size, bd, 300 + size[0] + bd)
            want = _blank(512, 256, bd)
            assert wu.predict(ref, want, desc, size[0], size[1], bd, 512, 256) == 0
            warp[(size, bd)] = (ref, desc, want)
        rng = np.random.default_rng(9)
        trefs = [ipu.random_picture(rng, 512, 256, ipu.border_for(16, 16), 8, kind) for kind in ("noise", "smooth")]
        tdesc = ipu.random_descs(rng, 300, 16, 16, 512, 256)
        twant = _blank(512, 256, 8)
        assert ipu.predict(trefs[0], trefs[1], twant, tdesc, 16, 16, 8) == 0

        def run_warp(key, step):
            ref, desc, want = warp[key]
            got, _ = wu.run_device(ctx, ref, _blank(512, 256, key[1]), desc, key[0][0], key[0][1], key[1], 512, 256)
            _compare(got, want, (step, key))

        def run_translational(step):
            got, _ = ipu.run_device(ctx, trefs[0], trefs[1], _blank(512, 256, 8), tdesc, 16, 16, 8)
            _compare(got, twant, (step, "translational"))

        keys = list(warp)
        run_warp(keys[0], "first")
        run_translational("after a warped call")
        run_warp(keys[1], "after a translational call")
        ctx.reserve(3840, 2160, 85, 1, host_forms=True)
        run_warp(keys[0], "after the 4K reserve")
        run_warp(keys[2], "after the 4K reserve")
        run_translational("after the 4K reserve")
        run_warp(keys[3], "grown list")
        run_warp(keys[0], "small again")
        run_translational("last")
        assert ctx.inter_pred_refused() == 0
    finally:
        ctx.close()
