#!/usr/bin/env python3
"""Times svthip_av1_[highbd_]warped_pred_batch_dev: one call per luma size for 1080p worth of PUs (1920 x 1088 / (w h) PUs; 16x16, 32x32 and
64x64 with warped chroma, 8x8 with translational chroma), 8 and 10 bits, against what existed before and is unchanged: the translational
whole-PU entry on the same PU positions with uni-predicted PUs (the same number of output samples), on its default path and on the VALU
path (OPT_CONVOLVE_VALU).

    python tools/warp_probe.py [--iters N] [--out FILE] [--sizes 16x16,...]

Times are device times in microseconds, measured by tools/probe_common.py: timed (median over N samples, each the mean of 10 back-to-back
calls queued behind a sleep kernel).  One JSON line per row; --out is overwritten.  For a kernel-trace pass:
rocprofv3 --kernel-trace --stats -- python tools/warp_probe.py."""
import argparse

import numpy as np

from probe_common import add_common_args, as_dev, emit, open_stream, timed, write_rows  # sets the import path

import inter_pred_probe as ipp  # noqa: E402  (the picture's size and the translational descriptors of the yardstick)
import inter_pred_util as ipu  # noqa: E402
import svtav1_hip  # noqa: E402
import warp_util as wu  # noqa: E402

W, H, BORDER = ipp.W, ipp.H, ipp.BORDER


def warp_descs_1080p(rng, bw, bh):
    """every bw x bh position of the picture; 64 random models of moderate size, block images within a few samples of the block"""
    ys, xs = np.mgrid[0:H // bh, 0:W // bw]
    x, y = (xs.reshape(-1) * bw), (ys.reshape(-1) * bh)
    n = len(x)
    d = np.zeros(n, svtav1_hip.WARP_PU_DESC_DTYPE)
    d["pu_origin_x"], d["pu_origin_y"], d["dst_origin_x"], d["dst_origin_y"] = x, y, x, y
    d["mb_to_left_edge"], d["mb_to_right_edge"] = -x * 8, (W - bw - x) * 8
    d["mb_to_top_edge"], d["mb_to_bottom_edge"] = -y * 8, (H - bh - y) * 8
    d["mv"] = rng.integers(-80, 81, (n, 2))
    d["has_uv"] = 1
    models = [wu.random_model(rng, wu.ROTZOOM if i & 1 else wu.AFFINE) for i in range(64)]
    pick = rng.integers(0, 64, n)
    mats = np.array([m for m, _ in models], np.int64)[pick]
    d["wmtype"] = np.where(pick & 1, wu.ROTZOOM, wu.AFFINE)
    for k, name in enumerate(("alpha", "beta", "gamma", "delta")):
        d[name] = np.array([s[k] for _, s in models])[pick]
    cx, cy = x + bw // 2, y + bh // 2
    tx, ty = cx + rng.integers(-10, 11, n), cy + rng.integers(-10, 11, n)
    d["wmmat"][:, 2:] = mats
    d["wmmat"][:, 0] = (tx << 16) + rng.integers(0, 1 << 16, n) - mats[:, 0] * cx - mats[:, 1] * cy
    d["wmmat"][:, 1] = (ty << 16) + rng.integers(0, 1 << 16, n) - mats[:, 2] * cx - mats[:, 3] * cy
    return d


def main():
    import torch
    ap = argparse.ArgumentParser()
    add_common_args(ap, 20)
    ap.add_argument("--sizes", default="8x8,16x16,32x32,64x64")
    ap.add_argument("--bit-depths", default="8,10")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    lines = []
    for bd in [int(v) for v in a.bit_depths.split(",")]:
        ref = ipu.random_picture(rng, W, H, BORDER, bd, "smooth")
        d_ref = ipu.to_device(ref)
        pred = ipu.Picture(*[np.zeros_like(p) for p in (ref.y, ref.cb, ref.cr)], BORDER)
        d_pred = ipu.to_device(pred)
        P0, PP = ipu.planes_of(d_ref, ref), ipu.planes_of(d_pred, pred)
        for bw, bh in [tuple(int(v) for v in t.split("x")) for t in a.sizes.split(",") if t]:
            wd = warp_descs_1080p(rng, bw, bh)
            td = ipp.descs_1080p(rng, bw, bh, "uni")   # pred_direction 0 / 1: one reference per PU, as the warp reads
            n = len(wd)
            d_wd, d_td = as_dev(torch, wd), as_dev(torch, td)
            if bd == 8:
                warp = lambda: ctx.av1_warped_pred_batch_dev(P0, PP, W, H, d_wd.data_ptr(), n, bw, bh, stream=stream)  # noqa: E731
                trans = lambda: ctx.av1_inter_pred_batch_dev(P0, P0, PP, d_td.data_ptr(), n, bw, bh, stream=stream)  # noqa: E731
            else:
                warp = lambda: ctx.av1_highbd_warped_pred_batch_dev(P0, PP, W, H, d_wd.data_ptr(), n, bw, bh, 10, stream=stream)  # noqa: E731
                trans = lambda: ctx.av1_highbd_inter_pred_batch_dev(P0, P0, PP, d_td.data_ptr(), n, bw, bh, 10, stream=stream)  # noqa: E731
            t_warp = timed(torch, warp, a.iters).median
            t_def = timed(torch, trans, a.iters).median
            ctx.set_option(svtav1_hip.OPT_CONVOLVE_VALU, 1)
            try:
                t_valu = timed(torch, trans, a.iters).median
            finally:
                ctx.set_option(svtav1_hip.OPT_CONVOLVE_VALU, 0)
            assert ctx.inter_pred_refused() == 0
            row = {"bd": bd, "size": f"{bw}x{bh}", "n_pu": n, "warped_us": round(t_warp, 2), "translational_us": round(t_def, 2),
                   "translational_valu_us": round(t_valu, 2), "ratio_vs_default": round(t_warp / t_def, 3), "ratio_vs_valu": round(t_warp / t_valu, 3)}
            emit(lines, row)
    ctx.close()
    write_rows(a.out, lines, append=False)


if __name__ == "__main__":
    main()
