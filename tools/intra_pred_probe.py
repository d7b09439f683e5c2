#!/usr/bin/env python3
"""Times svthip_av1_[highbd_]intra_pred_batch_dev: one call per transform size for a 1920 x 1088 picture's worth of blocks (4x4 .. 64x64),
mode mixes "dc" / "all13" / "directional", 8 and 10 bits, with and without d_sad, reading the edges straight from a padded plane
(above row y - 1, left column x - 1 at the plane stride) and writing the blocks to a second plane of the same layout.  Two yardsticks per row:
  bytes      the bytes the call must move (edges in, block out, source in when the SAD is asked) over the HBM rate DESIGN section 6 uses;
  copy_us    svthip_av1_[highbd_]inter_pred_batch_dev on the same block positions with zero vectors and luma only: the call the project
             already has that writes the same bytes (8x8 and above; that entry's descriptors for 4x4 carry chroma rules of their own).

    python tools/intra_pred_probe.py [--iters N] [--out FILE]

Times are device times in microseconds, the median tools/probe_common.py: timed gives.  One JSON line per row; --out is overwritten.
For a kernel-trace pass: rocprofv3 --kernel-trace --stats -- python tools/intra_pred_probe.py --iters 2."""
import argparse

import numpy as np

from probe_common import add_common_args, as_dev, emit, open_stream, timed, write_rows  # sets the import path

import inter_pred_probe as ipp  # noqa: E402  (the picture's size and the translational descriptors of the copy yardstick)
import inter_pred_util as ipu  # noqa: E402
import intra_pred_util as iu  # noqa: E402
import svtav1_hip  # noqa: E402

W, H, BORDER = ipp.W, ipp.H, ipp.BORDER
HBM_BYTES_PER_S = 8.0e12
MIXES = {"dc": [(0, 0)], "all13": [(m, 0) for m in range(13)], "directional": iu.DIRECTIONAL}


def intra_descs_1080p(rng, n_side, stride, origin, mix):
    """every n x n position; edges from the padded plane itself (all four counts full inside the border)"""
    ys, xs = np.mgrid[0:H // n_side, 0:W // n_side]
    x, y = xs.reshape(-1) * n_side + origin, ys.reshape(-1) * n_side + origin
    d = np.zeros(len(x), iu.DESC)
    d["above_offset"] = (y - 1) * stride + x
    d["left_offset"] = y * stride + x - 1
    d["left_stride"] = stride
    d["dst_offset"] = d["src_offset"] = y * stride + x
    d["dst_stride"] = d["src_stride"] = stride
    d["n_top_px"] = d["n_topright_px"] = d["n_left_px"] = d["n_bottomleft_px"] = n_side
    pick = rng.integers(0, len(MIXES[mix]), len(x))
    d["mode"] = np.array([m for m, _ in MIXES[mix]])[pick]
    d["angle_delta"] = np.array([a for _, a in MIXES[mix]])[pick]
    return d


def main():
    import torch
    ap = argparse.ArgumentParser()
    add_common_args(ap, 20)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    lines = []
    for bd in (8, 10):
        ref = ipu.random_picture(rng, W, H, BORDER, bd, "smooth")
        d_ref = ipu.to_device(ref)
        pred = ipu.Picture(*[np.zeros_like(p) for p in (ref.y, ref.cb, ref.cr)], BORDER)
        d_pred = ipu.to_device(pred)
        P0, PP = ipu.planes_of(d_ref, ref), ipu.planes_of(d_pred, pred)
        S = ref.y.shape[1]
        d_edge = d_ref["y"]          # the edges come from the reference plane, the blocks go to the prediction plane: same offsets
        d_dst = d_pred["y"]
        SB = 1 if bd == 8 else 2
        for tx_size, n_side in ((0, 4), (1, 8), (2, 16), (3, 32), (4, 64)):
            copy_us = None
            if n_side >= 8:
                td = ipp.descs_1080p(rng, n_side, n_side, "uni")
                td["mv"], td["interp_filters"], td["pred_direction"], td["own_list"], td["has_uv"] = 0, 0, 0, 0, 0
                d_td = as_dev(torch, td)
                if bd == 8:
                    trans = lambda: ctx.av1_inter_pred_batch_dev(P0, P0, PP, d_td.data_ptr(), len(td), n_side, n_side, stream=stream)  # noqa: E731
                else:
                    trans = lambda: ctx.av1_highbd_inter_pred_batch_dev(P0, P0, PP, d_td.data_ptr(), len(td), n_side, n_side, 10, stream=stream)  # noqa: E731
                copy_us = timed(torch, trans, a.iters).median
            for mix in MIXES:
                desc = intra_descs_1080p(rng, n_side, S, BORDER, mix)
                n = len(desc)
                d_desc = as_dev(torch, desc)
                d_sad = torch.zeros(n, dtype=torch.int32, device="cuda:0")
                for with_sad in ((False, True) if bd == 8 else (False,)):
                    if bd == 8:
                        fn = lambda: ctx.av1_intra_pred_batch_dev(d_edge.data_ptr(), d_dst.data_ptr(), d_desc.data_ptr(), n, tx_size,  # noqa: E731
                                                                  d_edge.data_ptr() if with_sad else None,
                                                                  d_sad.data_ptr() if with_sad else None, stream)
                    else:
                        fn = lambda: ctx.av1_highbd_intra_pred_batch_dev(d_edge.data_ptr(), d_dst.data_ptr(), d_desc.data_ptr(), n, tx_size, 10,  # noqa: E731
                                                                         stream)
                    t = timed(torch, fn, a.iters).median
                    nbytes = n * (SB * (4 * n_side + 1 + n_side * n_side * (2 if with_sad else 1)) + 32 + (4 if with_sad else 0))
                    floor_us = nbytes / HBM_BYTES_PER_S * 1e6
                    row = {"bd": bd, "size": f"{n_side}x{n_side}", "mix": mix, "sad": with_sad, "n_blocks": n, "intra_us": round(t, 2),
                           "bytes": nbytes, "hbm_floor_us": round(floor_us, 2), "ratio_vs_hbm_floor": round(t / floor_us, 2),
                           "copy_us": None if copy_us is None else round(copy_us, 2),
                           "ratio_vs_copy": None if copy_us is None else round(t / copy_us, 3)}
                    emit(lines, row)
        assert ctx.inter_pred_refused() == 0
    ctx.close()
    write_rows(a.out, lines, append=False)


if __name__ == "__main__":
    main()
