"""GPU: svthip_av1_[highbd_]inter_pred_batch_dev (whole-PU inter prediction, Y / Cb / Cr incl. sub-8x8 chroma) bit-exact against the
reference's fixture (tests/golden/inter_pred.npz), against the numpy restatement on random batches, and against the three per-plane
convolution entries fed with host-built descriptors; the caller-stream contract and every refusal."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import inter_pred_util as ipu  # noqa: E402
import svtav1_hip  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "inter_pred.npz")


def _compare(got, want, tag):
    for p in ("y", "cb", "cr"):
        g, w = getattr(got, p), getattr(want, p)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (tag, p, len(bad), bad[:4], g[tuple(bad[0])], w[tuple(bad[0])])


def _blank(pic_w, pic_h, bd, fill=None):
    dt = np.uint8 if bd == 8 else np.uint16
    f = (0x55 if bd == 8 else 0x155) if fill is None else fill
    return ipu.Picture(np.full((pic_h, pic_w), f, dt), np.full((pic_h // 2, pic_w // 2), f, dt), np.full((pic_h // 2, pic_w // 2), f, dt), 0)


@pytest.mark.parametrize("bd", [8, 10])
def test_fixture_bit_exact(hip_ctx, bd):
    pytest.importorskip("torch")
    from make_golden_inter_pred import PIC, reference_pictures
    g = dict(np.load(GOLDEN))
    refs = reference_pictures(bd)
    n_cases = 0
    for i in range(len(g["case_bw"])):
        if int(g["case_bd"][i]) != bd:
            continue
        bw, bh = int(g["case_bw"][i]), int(g["case_bh"][i])
        s, n = int(g["case_start"][i]), int(g["case_count"][i])
        desc = g["desc"][s:s + n].view(svtav1_hip.INTER_PU_DESC_DTYPE)
        got, _ = ipu.run_device(hip_ctx, refs[0], refs[1], _blank(PIC, PIC, bd), desc, bw, bh, bd)
        r = int(g["case_pred"][i])
        want = ipu.Picture(g[f"pred_y_{bd}"][r], g[f"pred_cb_{bd}"][r], g[f"pred_cr_{bd}"][r], 0)
        _compare(got, want, (i, bw, bh, bd))
        n_cases += 1
    assert n_cases > 22
    hip_ctx.inter_pred_refused()


def _random_batch(size, bd, seed, n_max=1500):
    bw, bh = size
    rng = np.random.default_rng(seed)
    pic_w, pic_h = 512, 256
    B = ipu.border_for(bw, bh)
    refs = [ipu.random_picture(rng, pic_w, pic_h, B, bd, kind) for kind in ("noise", "smooth")]
    n = min((pic_w // bw) * (pic_h // bh), n_max) - 3    # not a multiple of any workgroup's PU count: a partial last group
    desc = ipu.random_descs(rng, n, bw, bh, pic_w, pic_h, clamp_frac=0.2)
    return refs, desc, pic_w, pic_h


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", svtav1_hip.AV1_BLOCK_SIZES_WH)
def test_random_batches_match_restatement(hip_ctx, size, bd):
    pytest.importorskip("torch")
    bw, bh = size
    refs, desc, pic_w, pic_h = _random_batch(size, bd, bw * 1000 + bh * 10 + bd)
    assert set(desc["pred_direction"].tolist()) == {0, 1, 2}
    want = _blank(pic_w, pic_h, bd)
    assert ipu.predict(refs[0], refs[1], want, desc, bw, bh, bd) == 0
    got, _ = ipu.run_device(hip_ctx, refs[0], refs[1], _blank(pic_w, pic_h, bd), desc, bw, bh, bd)
    _compare(got, want, (size, bd))
    if (bw, bh) in ipu.SUB8_SIZES:   # the batch went through the piece kernel with every neighbour pattern
        used = [k for k in range(3) if (k == 0 and bw == 4 and bh == 4) or (k == 1 and bh == 4) or (k == 2 and bw == 4)]
        pats = {tuple(int(d["nb_is_inter"][k]) for k in used) for d in desc if d["has_uv"]}
        assert len(pats) == 1 << len(used)
        assert sum(ipu.sub8x8(d, bw, bh) for d in desc) > 10
    hip_ctx.inter_pred_refused()


def test_matrix_core_and_vector_kernels_agree(hip_ctx):
    """sides that are multiples of 32 run the luma / chroma jobs on the matrix-core kernel; the VALU option routes them to the other one"""
    pytest.importorskip("torch")
    for size in ((64, 64), (128, 64), (32, 32)):
        refs, desc, pic_w, pic_h = _random_batch(size, 8, 5 + size[0] + size[1])
        a, _ = ipu.run_device(hip_ctx, refs[0], refs[1], _blank(pic_w, pic_h, 8), desc, size[0], size[1], 8)
        hip_ctx.set_option(svtav1_hip.OPT_CONVOLVE_VALU, 1)
        try:
            b, _ = ipu.run_device(hip_ctx, refs[0], refs[1], _blank(pic_w, pic_h, 8), desc, size[0], size[1], 8)
        finally:
            hip_ctx.set_option(svtav1_hip.OPT_CONVOLVE_VALU, 0)
        _compare(a, b, size)


def _per_plane_reference(hip_ctx, refs, desc, bw, bh, bd, pic_w, pic_h):
    """The same prediction through the three per-plane entries with descriptors built on the host (clamp, integer / fraction split),
    one launch per plane and direction, as a caller of those entries does it (sizes >= 8x8: no sub-8x8 chroma; the entries apply the
    4-tap rule to their own block size)."""
    import torch
    out = _blank(pic_w, pic_h, bd)
    dev = {t: ipu.to_device(refs[t]) for t in range(2)}
    dp = ipu.to_device(out)
    bwu, bhu = max(4, bw >> 1), max(4, bh >> 1)
    for plane, (w, h), ss in (("y", (bw, bh), 0), ("cb", (bwu, bhu), 1), ("cr", (bwu, bhu), 1)):
        B = refs[0].border >> ss
        S = getattr(refs[0], plane).shape[1]
        D = getattr(out, plane).shape[1]
        for direction in (0, 1, 2):
            sel = desc[desc["pred_direction"] == direction]
            if len(sel) == 0:
                continue
            rows = []
            for d in sel:
                fx, fy = (int(d["interp_filters"]) >> 16) & 3, int(d["interp_filters"]) & 3
                ox = int(d["pu_origin_x"]) if not ss else ((int(d["pu_origin_x"]) >> 3) << 3) // 2
                oy = int(d["pu_origin_y"]) if not ss else ((int(d["pu_origin_y"]) >> 3) << 3) // 2
                dx = int(d["dst_origin_x"]) if not ss else ((int(d["dst_origin_x"]) >> 3) << 3) // 2
                dy = int(d["dst_origin_y"]) if not ss else ((int(d["dst_origin_y"]) >> 3) << 3) // 2
                offs, subs = [], []
                for l in ((0, 1) if direction == 2 else (direction,)):
                    r, c = ipu.clamp_mv(d, d["mv"][l][0], d["mv"][l][1], w, h, ss)
                    offs.append((B + oy + (r >> 4)) * S + B + ox + (c >> 4))
                    subs.append((c & 15, r & 15))
                if direction == 2:
                    rows.append((offs[0], offs[1], dy * D + dx, subs[0][0] | subs[0][1] << 4, subs[1][0] | subs[1][1] << 4, fx, fy))
                else:
                    rows.append((offs[0], dy * D + dx, subs[0][0], subs[0][1], fx, fy, 0))
            dt = svtav1_hip.CONVOLVE_COMPOUND_DESC_DTYPE if direction == 2 else svtav1_hip.CONVOLVE_DESC_DTYPE
            hd = np.array(rows, dt)
            d_desc = torch.from_numpy(hd.view(np.uint8).reshape(-1).copy()).to("cuda:0")
            src0, src1 = dev[0][plane].data_ptr(), dev[1][plane].data_ptr()
            dst = dp[plane].data_ptr()
            torch.cuda.synchronize()
            if bd == 8:
                if direction == 2:
                    hip_ctx.av1_convolve_compound_batch_dev(src0, S, src1, S, dst, D, d_desc.data_ptr(), len(hd), w, h)
                else:
                    hip_ctx.av1_convolve_sr_batch_dev(src0 if direction == 0 else src1, S, dst, D, d_desc.data_ptr(), len(hd), w, h)
            else:
                s = src0 if direction != 1 else src1
                _check_hbd(hip_ctx, s, S, src1, S, dst, D, d_desc.data_ptr(), int(direction == 2), len(hd), w, h)
            hip_ctx.synchronize()
    return ipu.Picture(dp["y"].cpu().numpy(), dp["cb"].cpu().numpy(), dp["cr"].cpu().numpy(), 0)


def _check_hbd(hip_ctx, s0, S0, s1, S1, dst, D, desc, compound, n, w, h):
    lib = svtav1_hip.lib()
    rc = lib.svthip_av1_highbd_convolve_batch_dev(hip_ctx._h, s0, S0, s1, S1, dst, D, desc, compound, n, w, h, 10, None)
    assert rc == 0, lib.svthip_last_error().decode()


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", [s for s in svtav1_hip.AV1_BLOCK_SIZES_WH if min(s) >= 8])
def test_equals_per_plane_entries(hip_ctx, size, bd):
    pytest.importorskip("torch")
    bw, bh = size
    refs, desc, pic_w, pic_h = _random_batch(size, bd, 31 * bw + bh + bd, n_max=600)
    got, _ = ipu.run_device(hip_ctx, refs[0], refs[1], _blank(pic_w, pic_h, bd), desc, bw, bh, bd)
    want = _per_plane_reference(hip_ctx, refs, desc, bw, bh, bd, pic_w, pic_h)
    _compare(got, want, (size, bd))


def test_caller_stream_without_synchronisation(hip_ctx):
    torch = pytest.importorskip("torch")
    for bd, size in ((8, (4, 4)), (10, (16, 8)), (8, (64, 64))):
        bw, bh = size
        refs, desc, pic_w, pic_h = _random_batch(size, bd, 900 + bd + bw)
        want = _blank(pic_w, pic_h, bd)
        ipu.predict(refs[0], refs[1], want, desc, bw, bh, bd)
        s = torch.cuda.Stream()
        d0, d1 = ipu.to_device(refs[0]), ipu.to_device(refs[1])
        dp = ipu.to_device(_blank(pic_w, pic_h, bd))
        d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        s.wait_stream(torch.cuda.current_stream())   # stream order, not a host wait
        args = (ipu.planes_of(d0, refs[0]), ipu.planes_of(d1, refs[1]), ipu.planes_of(dp, want), d_desc.data_ptr(), len(desc), bw, bh)
        with torch.cuda.stream(s):
            if bd == 8:
                hip_ctx.av1_inter_pred_batch_dev(*args, stream=s.cuda_stream)
            else:
                hip_ctx.av1_highbd_inter_pred_batch_dev(*args, bit_depth=10, stream=s.cuda_stream)
            host = {p: dp[p].to("cpu") for p in ("y", "cb", "cr")}   # enqueued on s behind the prediction
        got = ipu.Picture(host["y"].numpy(), host["cb"].numpy(), host["cr"].numpy(), 0)
        _compare(got, want, ("stream", size, bd))
    hip_ctx.inter_pred_refused()


def test_refusals(hip_ctx):
    torch = pytest.importorskip("torch")
    bw, bh, bd = 4, 4, 8
    refs, desc, pic_w, pic_h = _random_batch((bw, bh), bd, 4242, n_max=400)
    d0, d1 = ipu.to_device(refs[0]), ipu.to_device(refs[1])
    dp = ipu.to_device(_blank(pic_w, pic_h, bd))
    p0, p1, pp = ipu.planes_of(d0, refs[0]), ipu.planes_of(d1, refs[1]), ipu.planes_of(dp, _blank(pic_w, pic_h, bd))
    d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    n = len(desc)
    E = svtav1_hip.SvtHipError
    with pytest.raises(E, match="block size"):
        hip_ctx.av1_inter_pred_batch_dev(p0, p1, pp, d_desc.data_ptr(), n, 12, 12)
    with pytest.raises(E, match="block size"):
        hip_ctx.av1_inter_pred_batch_dev(p0, p1, pp, d_desc.data_ptr(), n, 4, 32)            # 8:1
    with pytest.raises(E, match="null"):
        hip_ctx.av1_inter_pred_batch_dev(None, p1, pp, d_desc.data_ptr(), n, bw, bh)
    with pytest.raises(E, match="null"):
        hip_ctx.av1_inter_pred_batch_dev(p0, p1, pp, None, n, bw, bh)
    hole = svtav1_hip.InterPlanes(p0.y, None, p0.cr, p0.y_stride, p0.c_stride)
    with pytest.raises(E, match="null"):
        hip_ctx.av1_inter_pred_batch_dev(hole, p1, pp, d_desc.data_ptr(), n, bw, bh)
    with pytest.raises(E, match="16-byte"):
        hip_ctx.av1_inter_pred_batch_dev(p0, p1, pp, buf.data_ptr() + 4, n, bw, bh)
    with pytest.raises(E, match="bit_depth"):
        hip_ctx.av1_highbd_inter_pred_batch_dev(p0, p1, pp, d_desc.data_ptr(), n, bw, bh, bit_depth=12)
    hip_ctx.av1_inter_pred_batch_dev(None, None, None, None, 0, bw, bh)                      # n_pu == 0: OK
    hip_ctx.inter_pred_refused()                                                            # nothing refused so far

    # BI_PRED PUs whose chroma goes sub-8x8: refused on the device, nothing written for them, counted
    bad = desc.copy()
    cand = [i for i, d in enumerate(bad) if d["has_uv"]][:7]
    for i in cand:
        bad[i]["pred_direction"] = 2
        bad[i]["nb_is_inter"][:] = 1
    want = _blank(pic_w, pic_h, bd)
    assert ipu.predict(refs[0], refs[1], want, bad, bw, bh, bd) == len(cand)
    got, _ = ipu.run_device(hip_ctx, refs[0], refs[1], _blank(pic_w, pic_h, bd), bad, bw, bh, bd)
    _compare(got, want, "bi-sub8")
    with pytest.raises(E, match=f"{len(cand)} PU"):
        hip_ctx.inter_pred_refused()
    hip_ctx.inter_pred_refused()                                                            # the count was cleared
