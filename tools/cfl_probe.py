#!/usr/bin/env python3
"""Times the three chroma-from-luma kernels on a 1920 x 1088 picture's worth of 16x16 luma blocks (8 160 blocks, chroma 8x8): the predict
entry at 8 and 10 bits (luma and DC prediction read from planes of the picture, the result written to a second pair of planes), the candidates entry (2 x 33 tiles per block into a pool) and the
decision kernel over the pool's 538 560 (distortion, bits) pairs.

    python tools/cfl_probe.py [--iters N] [--out FILE] [--only predict8,predict10,candidates,decision]

Times are device times in microseconds: the median over N samples, each the mean of 10 back-to-back calls queued behind a sleep kernel, as
tools/probe_common.py: timed takes them.  One JSON line per row; --out is overwritten.  "bytes" is what the call must move (luma, DC prediction and descriptor in, prediction out; for the
decision every pair and table it may read), "tb_s" that over the time, "hbm_share" that over the 8 TB/s peak DESIGN.md uses.
For a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/cfl_probe.py --iters 3"""
import argparse

import numpy as np

from probe_common import add_common_args, emit, open_stream, timed, write_rows  # sets the import path

import cfl_util as cu  # noqa: E402
import svtav1_hip  # noqa: E402

W, H, LW, LH = 1920, 1088, 16, 16
HBM_PEAK = 8e12


def picture_descs():
    """every 16x16 luma block of the picture, reading luma and chroma in place from planes of the picture's strides"""
    ys, xs = np.mgrid[0:H // LH, 0:W // LW]
    x, y = xs.reshape(-1) * LW, ys.reshape(-1) * LH
    d = np.zeros(len(x), cu.DESC)
    d["luma_offset"], d["luma_stride"] = y * W + x, W
    d["cb_offset"] = d["cr_offset"] = (y // 2) * (W // 2) + x // 2
    d["chroma_stride"] = W // 2
    rng = np.random.default_rng(3)
    for i in range(len(d)):
        d[i]["alpha_idx"], d[i]["alpha_signs"] = cu.alpha_to_fields(int(rng.integers(1, 17)), int(rng.integers(-16, 17)))
    return d


def main():
    import torch
    ap = argparse.ArgumentParser()
    add_common_args(ap, 20)
    ap.add_argument("--only", default="predict8,predict10,candidates,decision")
    a = ap.parse_args()
    only = set(a.only.split(","))
    rng = np.random.default_rng(1)
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    desc = picture_descs()
    n = len(desc)
    d_desc = cu.to_dev(desc)
    lines = []

    def report(name, fn, nbytes, **more):
        t = timed(torch, fn, a.iters).median
        row = {"kernel": name, "blocks": n, "us": round(t, 2), "bytes": int(nbytes), "tb_s": round(nbytes / t / 1e6, 3),
               "hbm_share": round(nbytes / (t * 1e-6) / HBM_PEAK, 4), **more}
        emit(lines, row)

    for bd in (8, 10):
        if f"predict{bd}" not in only and not (bd == 8 and "candidates" in only):
            continue
        dt, es = (np.uint8, 1) if bd == 8 else (np.uint16, 2)
        luma = rng.integers(0, 1 << bd, W * H).astype(dt)
        cb, cr = (np.repeat(rng.integers(0, 1 << bd, n), 64).astype(dt) for _ in range(2))   # any values: a timing run
        d_l, d_cb, d_cr = cu.to_dev(luma), cu.to_dev(cb), cu.to_dev(cr)
        d_ocb, d_ocr = torch.zeros_like(d_cb), torch.zeros_like(d_cr)
        if f"predict{bd}" in only:
            args = (d_l.data_ptr(), d_cb.data_ptr(), d_cr.data_ptr(), d_ocb.data_ptr(), d_ocr.data_ptr(), d_desc.data_ptr(), n, LW, LH)
            if bd == 8:
                call = lambda: ctx.av1_cfl_pred_batch_dev(*args, stream=stream)  # noqa: E731
            else:
                call = lambda: ctx.av1_highbd_cfl_pred_batch_dev(*args, 10, stream=stream)  # noqa: E731
            report(f"predict{bd}", call, n * (es * (LW * LH + 4 * 64) + 32))
        if bd == 8 and "candidates" in only:
            d_pool = torch.zeros(n * 66 * 64, dtype=torch.uint8, device="cuda:0")
            report("candidates", lambda: ctx.av1_cfl_alpha_candidates_batch_dev(d_l.data_ptr(), d_cb.data_ptr(), d_cr.data_ptr(), d_desc.data_ptr(),
                                                                                n, LW, LH, d_pool.data_ptr(), stream=stream),
                   n * (LW * LH + 2 * 64 + 32 + 66 * 64))
    if "decision" in only:
        ab = cu.random_alpha_bits(rng)
        dist, bits, jobs = cu.random_decision_tables(rng, 512)
        reps = (n + 511) // 512
        dist, bits, jobs = (np.concatenate([v] * reps)[:n] for v in (dist, bits, jobs))
        d2 = np.zeros((n * 66, 2), np.uint64)
        d2[:, 0] = dist.reshape(-1)
        d_d, d_b, d_a, d_j = cu.to_dev(d2), cu.to_dev(bits.reshape(-1)), cu.to_dev(ab), cu.to_dev(jobs)
        d_o = torch.zeros(n * cu.DECISION.itemsize, dtype=torch.uint8, device="cuda:0")
        report("decision", lambda: ctx.cfl_alpha_decision_batch_dev(d_d.data_ptr(), d_b.data_ptr(), 2, d_a.data_ptr(), d_j.data_ptr(), n,
                                                                    d_o.data_ptr(), stream=stream),
               n * (66 * (16 + 4) + 16 + 32) + ab.nbytes)
    ctx.inter_pred_refused()
    ctx.close()
    write_rows(a.out, lines, append=False)


if __name__ == "__main__":
    main()
