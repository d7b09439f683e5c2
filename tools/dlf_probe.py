#!/usr/bin/env python3
"""Times the deblocking entries on a 1920 x 1088 picture, 8 and 10 bits, with a mode-info grid that mixes 8x8 .. 64x64 blocks: the frame
filter of the three planes, one 64-level SSE table per plane, and the whole level pick (five tables and five walks).

    python tools/dlf_probe.py [--iters N] [--out FILE]

Times are device times in microseconds: the median over N samples, each the mean of back-to-back calls queued behind a sleep kernel, as
tools/probe_common.py: timed takes them.  One JSON line per row; --out is overwritten.  "bytes" is what the call must move (frame: every plane read and written once, and the grid; table:
the plane and its source read once, and the grid; pick: five tables), "tb_s" that over the time, "hbm_share" that over the 8 TB/s peak
DESIGN.md uses.  "ns_per_sample_level" of a table is its time over samples x 64 levels.  The frame filter works in place and a filtered
picture takes other branches than an unfiltered one, so every timed call is preceded by a device copy that restores the planes; the
copies alone are timed the same way and subtracted ("restore_us").  A CPU time of the reference is not part of the record: the reference
does not exist where this runs.
For a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/dlf_probe.py --iters 3
For the table kernel's vector instructions per sample and level: rocprofv3 --pmc SQ_INSTS_VALU -- python tools/dlf_probe.py --iters 1
--only table, in a run of its own; the counter counts wave instructions, so x 64 lanes / (samples x 64 levels) = the counter / samples."""
import argparse
import functools

import numpy as np

from probe_common import add_common_args, as_dev, emit, open_stream, timed, write_rows  # sets the import path

import dlf_util as du  # noqa: E402
import svtav1_hip  # noqa: E402

W, H = 1920, 1088
HBM_PEAK = 8e12


def main():
    import torch
    ap = argparse.ArgumentParser()
    add_common_args(ap, 10)
    ap.add_argument("--only", default="frame,table,pick")
    a = ap.parse_args()
    only = set(a.only.split(","))
    rng = np.random.default_rng(1)
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    mi = du.random_mi_grid(rng, W, H, min_size=8)
    dev = functools.partial(as_dev, torch)
    d_mi = dev(mi)
    d_levels = dev(np.array([24, 20, 16, 16], np.int32))
    d_sse = torch.zeros(5 * 64, dtype=torch.int64, device="cuda:0")
    lines = []

    def report(name, bd, fn, nbytes, reps, minus=0.0, **more):
        t = timed(torch, fn, a.iters, reps).median - minus
        if "samples" in more:
            more = {"ns_per_sample_level": round(t * 1e3 / (more["samples"] * 64), 5)}
        row = {"entry": name, "bit_depth": bd, "us": round(t, 1), "bytes": int(nbytes), "tb_s": round(nbytes / t / 1e6, 4),
               "hbm_share": round(nbytes / (t * 1e-6) / HBM_PEAK, 5), **more}
        emit(lines, row)

    for bd in (8, 10):
        es = 1 if bd == 8 else 2
        recon, source = du.random_picture(rng, W, H, bd, mi)
        d_rec, d_src = [dev(p) for p in recon], [dev(p) for p in source]
        pic = svtav1_hip.make_lf_picture(W, H, [d.data_ptr() for d in d_rec], [W, W // 2, W // 2], [d.data_ptr() for d in d_src], [W, W // 2, W // 2])
        samples = [W * H, W * H // 4, W * H // 4]
        d_keep = [d.clone() for d in d_rec]

        def restore():
            for d, k in zip(d_rec, d_keep):
                d.copy_(k, non_blocking=True)

        def frame():
            restore()
            ctx.av1_loop_filter_frame_dev(pic, d_mi.data_ptr(), mi.shape[1], d_levels.data_ptr(), 0, 0, 3, bit_depth=bd, stream=stream)

        if "frame" in only:
            t_restore = timed(torch, restore, a.iters, 10).median
            report("loop_filter_frame (3 planes)", bd, frame, 2 * sum(samples) * es + mi.nbytes, 10, minus=t_restore, restore_us=round(t_restore, 1))
            restore()
        for plane in range(3):
            if "table" in only:
                report(f"sse_table plane {plane}", bd,
                       lambda: ctx.av1_loop_filter_sse_table_dev(pic, d_mi.data_ptr(), mi.shape[1], plane, 2 if plane == 0 else 0, d_levels.data_ptr(),
                                                                 0, d_sse.data_ptr(), bit_depth=bd, stream=stream),
                       2 * samples[plane] * es + mi.nbytes, 3, samples=samples[plane])
        d_out = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        if "pick" in only:
            report("pick_filter_level (5 tables, 5 walks)", bd,
                   lambda: ctx.av1_pick_filter_level_dev(pic, d_mi.data_ptr(), mi.shape[1], (20, 20, 12, 12), 0, 0, d_out.data_ptr(), d_sse.data_ptr(),
                                                         bit_depth=bd, stream=stream),
                   2 * (3 * samples[0] + samples[1] + samples[2]) * es + 5 * mi.nbytes, 2)
    ctx.synchronize()
    ctx.close()
    write_rows(a.out, lines, append=False)


if __name__ == "__main__":
    main()
