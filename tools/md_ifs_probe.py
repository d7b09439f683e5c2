#!/usr/bin/env python3
"""Times mode decision's interpolation-filter search for one 1920 x 1080 picture's worth of candidates -- one per block, uni- and
bi-predicted mixed -- at three luma sizes, 8x8, 32x32 and 64x64, in the fast mode (search_mode 1 with the dual filter: trials 0, 3, 6):
  (i)   svthip_md_interp_filter_search_batch_dev, the whole call: trial descriptors, prediction, measurement, walk;
  (ii)  svthip_av1_inter_pred_batch_dev alone on the same 3 n trial descriptors (built on the host, the tiles in the grid the search uses);
  (iii) svthip_md_model_rd_batch_dev alone on those tiles, next to a device-to-device copy of the bytes it must read (the tiles and the
        source picture once);
  (iv)  the download of FIVE trial tiles per candidate to pageable host memory: what the reference's fast mode predicts per candidate (two
        of its five predictions repeat trial 0), so what a host-side search has to fetch when the predictions are made on the device;
  (v)   the reference's own interpolation_filter_search through tests/golden/ref_interp_search_driver.c on one host thread, on a sample of
        the same candidates, scaled to the picture (--reference: needs the reference, so it runs on the build machine, not on the GPU one).

    python tools/md_ifs_probe.py [--iters N] [--out FILE]        device times (needs a GPU)
    python tools/md_ifs_probe.py --reference [--out FILE]        row (v)
    python tools/md_ifs_probe.py --resources FILE                registers, LDS and scratch of the kernels from the compiler's remarks

Device times are microseconds per call: the median over N samples, each the mean of back-to-back calls queued behind a sleep kernel, as
tools/probe_common.py: timed takes them.  What was timed is compared with the restatement on a sample of candidates before it is reported.
One JSON line per row, appended to --out."""
import argparse
import functools
import tempfile
import time

import numpy as np

from probe_common import add_common_args, as_dev, emit, host_timed, open_stream, resources, timed, write_rows  # sets the import path

W, H, BORDER = 1920, 1080, 80
SIZES = (8, 32, 64)
QUANTIZER, TRIALS, REFERENCE_PREDICTIONS = 260, (0, 3, 6), 5


def pictures():
    """(ref0, ref1, src): padded smooth reference pictures with a little noise, the source close to reference 0"""
    import inter_pred_util as ipu
    rng = np.random.default_rng(5)

    def plane(w, h, b, phase):
        yy, xx = np.mgrid[0:h + 2 * b, 0:w + 2 * b + 32]
        return ((np.sin((xx + phase) / 7.0) + np.cos((yy - phase) / 5.0)) * 60 + 128 + rng.integers(-8, 9, xx.shape)).clip(0, 255).astype(np.uint8)

    refs = [ipu.Picture(plane(W, H, BORDER, p), plane(W // 2, H // 2, BORDER // 2, p + 3), plane(W // 2, H // 2, BORDER // 2, p + 5), BORDER) for p in (0, 2)]
    src = []
    for a, b in ((refs[0].y, BORDER), (refs[0].cb, BORDER // 2), (refs[0].cr, BORDER // 2)):
        h, w = a.shape[0] - 2 * b, a.shape[1] - 2 * b - 32
        src.append((a[b + 1:b + 1 + h, b + 1:b + 1 + w].astype(np.int32) + rng.integers(-4, 5, (h, w))).clip(0, 255).astype(np.uint8))
    return refs[0], refs[1], src


def candidates(size):
    """(INTER_PU_DESC_DTYPE[n], IFS_DESC_DTYPE[n]): one candidate per size x size block, vectors within 8 samples, directions mixed"""
    import md_ifs_util as mu
    import svtav1_hip
    rng = np.random.default_rng(size)
    nx, ny = W // size, H // size
    n = nx * ny
    pu, f = np.zeros(n, svtav1_hip.INTER_PU_DESC_DTYPE), np.zeros(n, mu.IFS_DESC_DTYPE)
    bx, by = np.meshgrid(np.arange(nx) * size, np.arange(ny) * size)
    x, y = bx.reshape(-1), by.reshape(-1)
    pu["pu_origin_x"], pu["pu_origin_y"] = x, y
    pu["mb_to_left_edge"], pu["mb_to_right_edge"] = -x * 8, (W - size - x) * 8
    pu["mb_to_top_edge"], pu["mb_to_bottom_edge"] = -y * 8, (H - size - y) * 8
    pu["pred_direction"] = rng.integers(0, 3, n)
    pu["has_uv"], pu["own_list"] = 1, pu["pred_direction"] == 1
    pu["mv"] = rng.integers(-64, 64, (n, 2, 2))
    f["src_x"], f["src_y"], f["lambda_"] = x, y, 3000
    f["filter_rate"] = rng.integers(20, 500, (n, 2, 3))
    return pu, f


def tile_grid(n_tiles, size):
    """(tiles per row, rows) of the grid the search lays its trial tiles out in"""
    rows_max = 65536 // size
    k = max(1, (n_tiles + rows_max - 1) // rows_max)
    return k, (n_tiles + k - 1) // k


def device_times(lines, iters):
    import torch

    import inter_pred_util as ipu
    import md_ifs_util as mu
    import svtav1_hip
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    ref0, ref1, src = pictures()
    pics = (ref0, ref1, ipu.Picture(*src, 0))
    dev = [ipu.to_device(p) for p in pics]
    P = [ipu.planes_of(d, p) for d, p in zip(dev, pics)]
    upload = functools.partial(as_dev, torch)

    def report(name, us, size, n, kind="device events", **more):
        emit(lines, {"entry": name, "kind": kind, "width": W, "height": H, "block": f"{size}x{size}", "candidates": n, "us": round(us, 1), **more})

    for size in SIZES:
        pu, f = candidates(size)
        n = len(pu)
        d_pu, d_f = upload(pu), upload(f)
        d_result = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
        search = lambda: ctx.md_interp_filter_search_batch_dev(P[0], P[1], P[2], d_pu.data_ptr(), d_f.data_ptr(), n, size, size, 1, 1, QUANTIZER, 0,  # noqa: E731
                                                               d_result.data_ptr(), stream=stream)
        t_search = timed(torch, search, iters, 5).median
        torch.cuda.synchronize()
        got = d_result.cpu().numpy().view(mu.IFS_RESULT_DTYPE)
        some = np.arange(0, n, max(1, n // 40))
        trials = [mu.Trials(ref0, ref1, src, pu[k], f[k], size, size, QUANTIZER) for k in some]
        assert np.array_equal(got[some], mu.search(trials, 1, 1)[0]), "the timed search differs from the restatement"
        assert ctx.inter_pred_refused() == 0

        # the same trials from the host's side: descriptors, a tile picture in the search's grid, the measurement's descriptors
        n_tiles = n * len(TRIALS)
        k, rows = tile_grid(n_tiles, size)
        t_pu = np.repeat(pu, len(TRIALS))
        t = np.arange(n_tiles)
        t_pu["interp_filters"] = np.tile([mu.trial_filters(i) for i in TRIALS], n)
        t_pu["dst_origin_x"], t_pu["dst_origin_y"] = (t % k) * size, (t // k) * size
        m = np.zeros(n_tiles, mu.MODEL_DESC_DTYPE)
        m["src_x"], m["src_y"], m["pred_x"], m["pred_y"] = np.repeat(f["src_x"], 3), np.repeat(f["src_y"], 3), t_pu["dst_origin_x"], t_pu["dst_origin_y"]
        m["lambda_"], m["rate"] = 3000, 100
        tiles = ipu.Picture(np.zeros((rows * size, k * size), np.uint8), *(np.zeros((rows * size // 2, k * size // 2), np.uint8) for _ in range(2)), 0)
        d_tiles = ipu.to_device(tiles)
        p_tiles = ipu.planes_of(d_tiles, tiles)
        d_tpu, d_m = upload(t_pu), upload(m)
        d_mres = torch.zeros(n_tiles * 32, dtype=torch.uint8, device="cuda:0")
        predict = lambda: ctx.av1_inter_pred_batch_dev(P[0], P[1], p_tiles, d_tpu.data_ptr(), n_tiles, size, size, stream=stream)  # noqa: E731
        measure = lambda: ctx.md_model_rd_batch_dev(P[2], p_tiles, d_m.data_ptr(), n_tiles, size, size, QUANTIZER, d_mres.data_ptr(), stream=stream)  # noqa: E731
        t_predict = timed(torch, predict, iters, 5).median
        t_measure = timed(torch, measure, iters, 10).median
        torch.cuda.synchronize()
        got_m = d_mres.cpu().numpy().view(mu.MODEL_RESULT_DTYPE)
        for j, c in zip(range(len(some)), some):
            assert int(got_m[c * 3 + 1]["sse"].sum()) == trials[j](3)[1], "the timed measurement differs from the restatement"
        assert ctx.inter_pred_refused() == 0
        # yardsticks: a copy of what the measurement reads; the download of five tiles a candidate
        sources = [d_tiles["y"], d_tiles["cb"], d_tiles["cr"], dev[2]["y"], dev[2]["cb"], dev[2]["cr"]]
        copies = [torch.empty_like(s) for s in sources]
        t_copy = timed(torch, lambda: [d.copy_(s) for d, s in zip(copies, sources)], iters, 10).median
        read = sum(s.numel() for s in sources) + m.nbytes
        five = torch.zeros(n * REFERENCE_PREDICTIONS * size * size * 3 // 2, dtype=torch.uint8, device="cuda:0")
        host = torch.empty(five.shape, dtype=torch.uint8)
        t_down = host_timed(lambda: (host.copy_(five), torch.cuda.synchronize()), iters, torch.cuda.synchronize).median
        report("(i) interpolation-filter search, fast mode, whole call", t_search, size, n, trials_per_candidate=3, search_minus_prediction_over_prediction=round((t_search - t_predict) / t_predict, 2),
               download_over_search=round(t_down / t_search, 1))
        report("(ii) inter prediction alone on the same trial descriptors", t_predict, size, n, pus=n_tiles)
        report("(iii) model-rd measurement alone on the trial tiles", t_measure, size, n, tiles=n_tiles, bytes=read, GB_per_s=round(read / t_measure / 1e3, 1),
               measure_over_copy=round(t_measure / t_copy, 2))
        report("(iii) yardstick: device-to-device copy of the trial tiles and the source picture", t_copy, size, n, bytes=read - m.nbytes,
               GB_per_s=round((read - m.nbytes) / t_copy / 1e3, 1))
        report("(iv) yardstick: download of five trial tiles per candidate to pageable host memory", t_down, size, n, kind="host clock around a synchronous copy",
               bytes=five.numel(), GB_per_s=round(five.numel() / t_down / 1e3, 1))
    ctx.synchronize()
    ctx.close()


def reference_times(lines, sample=60, repeat=200):
    """row (v): the reference's function on one host thread, `sample` candidates spread over the picture, each called `repeat` times"""
    import make_golden_md_ifs as gen
    ref0, ref1, src = pictures()
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(tmp)
        for size in SIZES:
            pu, f = candidates(size)
            n = len(pu)
            some = np.arange(0, n, max(1, n // sample))
            for k in some[:3]:
                gen.reference_search(L, (ref0, ref1, src), pu[k], f[k], size, size, QUANTIZER, 1, 1)
            t0 = time.perf_counter()
            for k in some:
                gen.reference_search(L, (ref0, ref1, src), pu[k], f[k], size, size, QUANTIZER, 1, 1, repeat=repeat)
            one = (time.perf_counter() - t0) / (len(some) * repeat)
            row = {"entry": "(v) reference interpolation_filter_search, fast mode, one host thread (C kernels), scaled to the picture",
                   "kind": "host clock, build machine", "width": W, "height": H, "block": f"{size}x{size}", "candidates": n, "us": round(one * n * 1e6, 1),
                   "us_per_candidate": round(one * 1e6, 2), "sampled": int(len(some))}
            emit(lines, row)


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 7, resources=True)
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    if a.resources:
        return resources("md_ifs.hip", a.resources, spill=True)
    lines = []
    if a.reference:
        reference_times(lines)
    else:
        device_times(lines, a.iters)
    write_rows(a.out, lines)


if __name__ == "__main__":
    main()
