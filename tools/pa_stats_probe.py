#!/usr/bin/env python3
"""Times the picture-analysis statistics entries on 12 synthetic 1920 x 1080 pictures per launch (510 SBs each, 30 x 17, the last row 56
high), BLOCK_MEAN_PREC_SUB and _FULL: svthip_pa_block_stats_dev, svthip_pa_homogeneity_dev, svthip_pa_histograms_dev, and next to them in the
same run the two yardsticks: a device-to-device copy of as many bytes as the block statistics read (what a one-pass read kernel can hope for),
and the download the three entries replace, the planes they read (luma and both chroma planes, 3.1 MB a picture) copied to pageable host memory.

    python tools/pa_stats_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/pa_stats_probe.py --cpu [--out FILE]                the CPU yardstick (build container only, where the reference exists)
    python tools/pa_stats_probe.py --resources FILE                  registers, LDS and scratch of the kernels from the compiler's remarks

Device times are microseconds per LAUNCH of 12 pictures: the median over N samples, each the mean of back-to-back calls queued behind a sleep
kernel, as tools/probe_common.py: timed takes them; bytes are what the algorithm reads, computed from the shapes below, and GB/s is bytes over that
time.  The download is timed by the host clock around synchronous copies.  --cpu times the reference's own GatheringPictureStatistics (with its
edge-detection tail, which the device entries leave to the host) on one picture, one thread, through the fixture driver
(tests/golden/ref_pa_stats_driver.c, ASM_AVX2): microseconds per picture, best of five runs of 20 calls.  One JSON line per row, appended to --out.
For a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/pa_stats_probe.py --iters 2"""
import argparse
import tempfile

import numpy as np

from probe_common import add_common_args, emit, host_timed, open_stream, resources, timed, write_rows  # sets the import path

W, H, N_PICS = 1920, 1080, 12


def picture(seed):
    """a moving texture with flat and noisy patches: (luma, cb, cr)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    luma = (128 + 60 * np.sin((x + 3 * seed) / 37.0) * np.cos((y - seed) / 23.0) + rng.integers(-6, 7, (H, W)) * ((x // 64 + y // 64) % 3 == 0)).clip(0, 255)
    luma = luma.astype(np.uint8)
    return luma, np.ascontiguousarray(luma[::2, ::2]), np.ascontiguousarray(255 - luma[1::2, 1::2])


def bytes_read():
    """what each entry has to read of one picture"""
    import pa_stats_util as pu
    nx, ny = pu.sb_grid(W, H)
    complete = int(pu.complete_sbs(W, H).sum())
    chroma_hist = sum(pu.region_geometry(W, H, 1, rx, ry)[2] * pu.region_geometry(W, H, 1, rx, ry)[3] for rx in range(4) for ry in range(4))
    return {"block_stats_full": nx * ny * 4096 + complete * 2 * 1024, "block_stats_sub": nx * ny * 2048 + complete * 2 * 512,
            "homogeneity": nx * ny * 85 * 2, "histograms": (W >> 2) * (H >> 2) + 2 * chroma_hist, "planes": W * H * 3 // 2}


def cpu_yardstick(lines):
    import make_golden_pa_stats as gen
    assert gen.reference_available(), "the CPU yardstick needs the reference sources and oracle/_ref/obj_all"
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(tmp)
        keep = [np.ascontiguousarray(p) for p in picture(0)]
        assert L.drv_pa_stats_open(W, H, *[p.ctypes.data for p in keep]) == 510
        for sub in (1, 0):
            t = min(L.drv_pa_stats_time(sub, 20) for _ in range(5)) / 20
            emit(lines, {"entry": "reference GatheringPictureStatistics, 1 picture, 1 thread", "kind": "cpu, build container, host clock",
                         "sub_precision": sub, "us": round(t * 1e6, 1)})
        L.drv_pa_stats_close()


def device_times(lines, iters):
    import torch

    import pa_stats_util as pu
    import svtav1_hip
    from svtav1_hip import synth
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    planes = [picture(s) for s in range(N_PICS)]
    luma_pool, descs = svtav1_hip.build_picture_pool([synth.PaPicture(p[0]) for p in planes])
    cstride, cbytes = W // 2, (W // 2) * (H // 2)
    pool = np.concatenate([luma_pool] + [c.reshape(-1) for p in planes for c in p[1:]] + [np.zeros(256, np.uint8)])
    offsets = [[luma_pool.size + (2 * i + k) * cbytes for k in (0, 1)] for i in range(N_PICS)]
    d_pool = torch.from_numpy(pool).to("cuda:0")
    n_sb = pu.sb_grid(W, H)[0] * pu.sb_grid(W, H)[1]
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")  # noqa: E731
    d_y, d_var, d_cb, d_cr = z((N_PICS, n_sb, 85), torch.uint8), z((N_PICS, n_sb, 85), torch.int16), z((N_PICS, n_sb, 21), torch.uint8), z((N_PICS, n_sb, 21), torch.uint8)
    d_vov, d_hom, d_pic = z((N_PICS, n_sb, 4), torch.int64), z((N_PICS, n_sb), torch.uint8), z((N_PICS, 4), torch.int32)
    d_hist, d_reg, d_avg = z((N_PICS, 4, 4, 3, 256), torch.int32), z((N_PICS, 4, 4, 3), torch.int32), z((N_PICS, 3), torch.int32)
    B = bytes_read()
    torch.cuda.synchronize()

    def report(name, fn, reps, nbytes, **more):
        us = timed(torch, fn, iters, reps).median
        emit(lines, {"entry": name, "kind": "device events", "pictures": N_PICS, "us": round(us, 1), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1), **more})
        return us

    total = {}
    for sub in (1, 0):
        key = "block_stats_sub" if sub else "block_stats_full"
        total[sub] = report(f"pa_block_stats ({'SUB' if sub else 'FULL'})", lambda: ctx.pa_block_stats_dev(
            d_pool.data_ptr(), descs, offsets, cstride, sub, d_y.data_ptr(), d_var.data_ptr(), d_cb.data_ptr(), d_cr.data_ptr(), stream=stream), 10, N_PICS * B[key])
    # correctness of what was timed, on the first and last picture
    torch.cuda.synchronize()
    for i in (0, N_PICS - 1):
        want = pu.block_stats(*planes[i], 0)
        got = (d_y[i].cpu().numpy(), d_var[i].cpu().numpy().view(np.uint16), d_cb[i].cpu().numpy(), d_cr[i].cpu().numpy())
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "the timed block statistics differ from the restatement"
    t_hom = report("pa_homogeneity", lambda: ctx.pa_homogeneity_dev(d_var.data_ptr(), W, H, N_PICS, d_vov.data_ptr(), d_hom.data_ptr(), d_pic.data_ptr(),
                                                                    stream=stream), 10, N_PICS * B["homogeneity"])
    t_hist = report("pa_histograms", lambda: ctx.pa_histograms_dev(d_pool.data_ptr(), descs, offsets, cstride, d_hist.data_ptr(), d_reg.data_ptr(),
                                                                   d_avg.data_ptr(), stream=stream), 10, N_PICS * B["histograms"])
    for sub in (1, 0):
        key = "block_stats_sub" if sub else "block_stats_full"
        src = torch.zeros(N_PICS * B[key], dtype=torch.uint8, device="cuda:0")
        dst = torch.zeros_like(src)
        report(f"yardstick: device-to-device copy of the bytes pa_block_stats ({'SUB' if sub else 'FULL'}) reads", lambda: dst.copy_(src), 10, N_PICS * B[key])
    # the download the entries replace: pageable host memory, synchronous, host clock
    for n in (1, N_PICS):
        dev = torch.zeros(n * B["planes"], dtype=torch.uint8, device="cuda:0")
        host = torch.zeros(n * B["planes"], dtype=torch.uint8)
        us = host_timed(lambda: (host.copy_(dev), torch.cuda.synchronize()), iters, torch.cuda.synchronize).median
        emit(lines, {"entry": f"yardstick: download of the planes of {n} picture(s) to pageable host memory", "kind": "host clock around synchronous copies",
                     "pictures": n, "us": round(us, 1), "bytes": n * B["planes"], "GB_per_s": round(n * B["planes"] / us / 1e3, 1)})
    download_us = lines[-1]["us"]   # of all N_PICS pictures
    for sub in (1, 0):
        emit(lines, {"entry": f"the three entries together ({'SUB' if sub else 'FULL'})", "kind": "sum of the device times above", "pictures": N_PICS,
                     "us": round(total[sub] + t_hom + t_hist, 1), "download_us": download_us,
                     "cheaper_than_the_download": total[sub] + t_hom + t_hist < download_us})
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 7, cpu=True, resources=True)
    a = ap.parse_args()
    lines = []
    if a.resources:
        return resources("pa_stats.hip", a.resources)
    if a.cpu:
        cpu_yardstick(lines)
    else:
        device_times(lines, a.iters)
    write_rows(a.out, lines)


if __name__ == "__main__":
    main()
