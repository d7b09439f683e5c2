#!/usr/bin/env python3
"""Times svthip_av1_inter_pred_batch_dev: one call per luma size for 1080p worth of PUs (1920 x 1088 / (w h) PUs, mixed directions, 8-bit
and 10-bit), plus two 4x4 batches whose chroma is all sub-8x8 (the piece kernel) or all 4x4 (a neighbour intra: the convolution kernel).
For sizes >= 8x8 the same work also goes through the three per-plane entries with descriptors built on the host beforehand (one launch
per plane and direction group, what a caller of those entries launches); only the device time of the launches is measured.

    python tools/inter_pred_probe.py [--iters N] [--out FILE]

Times are device times in microseconds: the median over N samples, each the mean of 10 back-to-back calls queued behind a sleep kernel
(tools/probe_common.py: timed).  One JSON line per row; --out is overwritten.
--sizes limits the run (e.g. for a kernel-trace pass: rocprofv3 --kernel-trace --stats -- python tools/inter_pred_probe.py --sizes 4x4,8x8)."""
import argparse

import numpy as np

from probe_common import add_common_args, as_dev, emit, open_stream, timed, write_rows  # sets the import path

import inter_pred_util as ipu  # noqa: E402
import svtav1_hip  # noqa: E402

W, H, BORDER = 1920, 1088, 144


def descs_1080p(rng, bw, bh, mode="mixed"):
    """every bw x bh position of the picture, vectorised (random vectors within +-10 samples, a few clamped, every filter pair)"""
    ys, xs = np.mgrid[0:H // bh, 0:W // bw]
    x, y = (xs.reshape(-1) * bw), (ys.reshape(-1) * bh)
    n = len(x)
    d = np.zeros(n, svtav1_hip.INTER_PU_DESC_DTYPE)
    d["pu_origin_x"], d["pu_origin_y"], d["dst_origin_x"], d["dst_origin_y"] = x, y, x, y
    d["mb_to_left_edge"], d["mb_to_right_edge"] = -x * 8, (W - bw - x) * 8
    d["mb_to_top_edge"], d["mb_to_bottom_edge"] = -y * 8, (H - bh - y) * 8
    d["interp_filters"] = (rng.integers(0, 4, n) << 16) | rng.integers(0, 4, n)
    d["mv"] = rng.integers(-80, 81, (n, 2, 2))
    d["nb_mv"] = rng.integers(-80, 81, (n, 3, 2))
    d["nb_list"] = rng.integers(0, 2, (n, 3))
    d["has_uv"] = [ipu.geometry_has_uv(bw, bh, int(a), int(b)) for a, b in zip(x, y)] if (bw == 4 or bh == 4) else 1
    if mode == "mixed":
        d["pred_direction"] = rng.integers(0, 3, n)
        d["nb_is_inter"] = 1
        d["nb_is_inter"][d["pred_direction"] == 2, 2 if bw == 4 else 1] = 0   # no BI_PRED PU goes sub-8x8
    else:
        d["pred_direction"] = rng.integers(0, 2, n)
        d["nb_is_inter"] = 1 if mode == "sub8" else 0
    d["own_list"] = d["pred_direction"] == 1
    return d


def per_plane_jobs(desc, bw, bh, ys, cs):
    """host-built descriptors of the per-plane entries: {(plane kind, direction): array}"""
    bwu, bhu = max(4, bw >> 1), max(4, bh >> 1)
    out = {}
    for kind, (w, h), ss, S, B in (("y", (bw, bh), 0, ys, BORDER), ("c", (bwu, bhu), 1, cs, BORDER // 2)):
        for direction in (0, 1, 2):
            sel = desc[desc["pred_direction"] == direction]
            if len(sel) == 0:
                continue
            rows = []
            for d in sel:
                f = int(d["interp_filters"])
                fx, fy = (f >> 16) & 3, f & 3
                ox, oy = (int(d["pu_origin_x"]), int(d["pu_origin_y"])) if not ss else \
                    (((int(d["pu_origin_x"]) >> 3) << 3) // 2, ((int(d["pu_origin_y"]) >> 3) << 3) // 2)
                offs, subs = [], []
                for l in ((0, 1) if direction == 2 else (direction,)):
                    r, c = ipu.clamp_mv(d, d["mv"][l][0], d["mv"][l][1], w, h, ss)
                    offs.append((B + oy + (r >> 4)) * S + B + ox + (c >> 4))
                    subs.append((c & 15) | ((r & 15) << 4))
                if direction == 2:
                    rows.append((offs[0], offs[1], oy * S + ox, subs[0], subs[1], fx, fy))  # prediction planes: same layout
                else:
                    rows.append((offs[0], oy * S + ox, subs[0] & 15, subs[0] >> 4, fx, fy, 0))
            out[(kind, direction)] = np.array(rows, svtav1_hip.CONVOLVE_COMPOUND_DESC_DTYPE if direction == 2 else svtav1_hip.CONVOLVE_DESC_DTYPE)
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    add_common_args(ap, 20)
    ap.add_argument("--per-plane-max-pus", type=int, default=40000, help="skip the per-plane comparison above this many PUs (host build time)")
    ap.add_argument("--sizes", default="", help="comma-separated WxH list (default: all 22)")
    ap.add_argument("--bit-depths", default="8,10")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    lines = []
    only = {tuple(int(v) for v in t.split("x")) for t in a.sizes.split(",") if t}
    for bd in [int(v) for v in a.bit_depths.split(",")]:
        refs = [ipu.random_picture(rng, W, H, BORDER, bd, "smooth") for _ in range(2)]
        d_refs = [ipu.to_device(r) for r in refs]
        pred = ipu.Picture(*[np.zeros_like(p) for p in (refs[0].y, refs[0].cb, refs[0].cr)], BORDER)
        d_pred = ipu.to_device(pred)
        P0, P1, PP = ipu.planes_of(d_refs[0], refs[0]), ipu.planes_of(d_refs[1], refs[1]), ipu.planes_of(d_pred, pred)
        cases = [(s, "mixed") for s in ipu.SIZES] + [((4, 4), "sub8"), ((4, 4), "c4x4")]
        for (bw, bh), mode in cases:
            if only and (bw, bh) not in only:
                continue
            desc = descs_1080p(rng, bw, bh, mode)
            d_desc = as_dev(torch, desc)
            n = len(desc)
            if bd == 8:
                call = lambda: ctx.av1_inter_pred_batch_dev(P0, P1, PP, d_desc.data_ptr(), n, bw, bh, stream=stream)  # noqa: E731
            else:
                call = lambda: ctx.av1_highbd_inter_pred_batch_dev(P0, P1, PP, d_desc.data_ptr(), n, bw, bh, 10, stream=stream)  # noqa: E731
            t_pu = timed(torch, call, a.iters).median
            ctx.inter_pred_refused()
            row = {"bd": bd, "size": f"{bw}x{bh}", "mode": mode, "n_pu": n, "whole_pu_us": round(t_pu, 2)}
            if min(bw, bh) >= 8 and mode == "mixed" and n <= a.per_plane_max_pus:
                jobs = per_plane_jobs(desc, bw, bh, refs[0].y.shape[1], refs[0].cb.shape[1])
                dj = {k: as_dev(torch, v) for k, v in jobs.items()}
                bwu, bhu = max(4, bw >> 1), max(4, bh >> 1)
                lib = svtav1_hip.lib()

                def planes_call():
                    for (kind, direction), t in dj.items():
                        w, h = (bw, bh) if kind == "y" else (bwu, bhu)
                        for p in (("y",) if kind == "y" else ("cb", "cr")):
                            s0, s1 = d_refs[0][p].data_ptr(), d_refs[1][p].data_ptr()
                            S = refs[0].y.shape[1] if kind == "y" else refs[0].cb.shape[1]
                            dst = d_pred[p].data_ptr() + ((BORDER if kind == "y" else BORDER // 2) * (S) +
                                                          (BORDER if kind == "y" else BORDER // 2)) * (1 if bd == 8 else 2)
                            cnt = len(jobs[(kind, direction)])
                            if bd == 8 and direction == 2:
                                rc = lib.svthip_av1_convolve_compound_batch_dev(ctx._h, s0, S, s1, S, dst, S, t.data_ptr(), cnt, w, h, stream)
                            elif bd == 8:
                                rc = lib.svthip_av1_convolve_sr_batch_dev(ctx._h, s1 if direction == 1 else s0, S, dst, S, t.data_ptr(), cnt, w, h, stream)
                            else:
                                rc = lib.svthip_av1_highbd_convolve_batch_dev(ctx._h, s1 if direction == 1 else s0, S, s1, S, dst, S, t.data_ptr(),
                                                                              int(direction == 2), cnt, w, h, 10, stream)
                            assert rc == 0, lib.svthip_last_error().decode()

                t_pp = timed(torch, planes_call, a.iters).median
                row.update(per_plane_us=round(t_pp, 2), ratio=round(t_pu / t_pp, 3), per_plane_launches=sum(1 if k[0] == "y" else 2 for k in jobs))
            emit(lines, row)
    ctx.close()
    write_rows(a.out, lines, append=False)


if __name__ == "__main__":
    main()
