#!/usr/bin/env python3
"""Times input-picture noise detection and denoising on 12 synthetic 1920 x 1080 pictures per launch (510 SBs each, 480 complete):
svthip_pa_noise_detect_dev without d_denoised (detection only, the configuration of the reference's encoder) and with it, both precisions,
and svthip_pa_denoise_dev in its whole-picture arm (class 3_1: every picture's luma copied back, both chroma planes filtered), and next to
them in the same run a device-to-device copy of as many bytes as the detection reads plus writes (what a one-pass kernel can hope for; the copy
moves each of them twice) and
the download of the planes that a host-side detection would cost (profiles/pa_stats_probe.jsonl records it for the same planes).

    python tools/pa_noise_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/pa_noise_probe.py --cpu [--out FILE]                the CPU yardstick (build container only, where the reference exists)
    python tools/pa_noise_probe.py --resources FILE                  registers, LDS and scratch of the kernels from the compiler's remarks

Device times are microseconds per LAUNCH of 12 pictures: the median over N samples, each the mean of back-to-back calls queued behind a sleep
kernel, as tools/probe_common.py: timed takes them; bytes are what the algorithm reads and writes, computed from the shapes below, and GB/s is
bytes over that time.  --cpu times the reference's own FullSampleDenoise with denoiseFlag 0 on one picture, one thread, through the fixture
driver (tests/golden/ref_pa_noise_driver.c, ASM_AVX2): microseconds per picture, best of five runs of 10 calls.  One JSON line per row,
appended to --out.  For a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/pa_noise_probe.py --iters 2"""
import argparse
import tempfile

import numpy as np

from probe_common import add_common_args, emit, host_timed, open_stream, resources, timed, write_rows  # sets the import path

W, H, N_PICS = 1920, 1080, 12


def picture(seed):
    """flat 128 with noise of a few levels everywhere, strong enough for class 3_1 at this height (noiseTh = 0): (luma, cb, cr)"""
    rng = np.random.default_rng(seed)
    luma = (128 + rng.integers(-24, 25, (H, W))).astype(np.uint8)
    return luma, np.ascontiguousarray(luma[::2, ::2]), np.ascontiguousarray(255 - luma[1::2, 1::2])


def bytes_moved():
    """of one picture: what detection reads (every SB with its one-sample halo, the stored halo 4 samples wide) and writes"""
    import pa_stats_util as pu
    n_sb = pu.sb_grid(W, H)[0] * pu.sb_grid(W, H)[1]
    return {"luma": W * H, "tables": n_sb * 17 + 16, "planes": W * H * 3 // 2}


def cpu_yardstick(lines):
    import make_golden_pa_noise as gen
    assert gen.reference_available(), "the CPU yardstick needs the reference sources and oracle/_ref/obj_all"
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(tmp)
        keep = [np.ascontiguousarray(p) for p in picture(0)]
        assert L.drv_pa_noise_open(W, H, *[p.ctypes.data for p in keep]) == 510
        for sub in (1, 0):
            t = min(L.drv_pa_noise_time(sub, 10) for _ in range(5)) / 10
            emit(lines, {"entry": "reference FullSampleDenoise (denoiseFlag 0), 1 picture, 1 thread", "kind": "cpu, build container, host clock",
                         "sub_precision": sub, "us": round(t * 1e6, 1)})
        L.drv_pa_noise_close()


def device_times(lines, iters):
    import torch

    import pa_noise_util as nu
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
    d_den, d_var, d_flat, d_pic = z((N_PICS, H, W), torch.uint8), z((N_PICS, n_sb, 2), torch.int64), z((N_PICS, n_sb), torch.uint8), z((N_PICS, 4), torch.int32)
    B = bytes_moved()
    torch.cuda.synchronize()

    def report(name, fn, reps, nbytes, **more):
        us = timed(torch, fn, iters, reps).median
        emit(lines, {"entry": name, "kind": "device events", "pictures": N_PICS, "us": round(us, 1), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1), **more})
        return us

    detect_us = {}
    for sub in (1, 0):
        for write in (False, True):
            nbytes = N_PICS * (B["luma"] * (2 if write else 1) + B["tables"])
            detect_us[(sub, write)] = report(f"pa_noise_detect ({'SUB' if sub else 'FULL'}, {'with' if write else 'without'} d_denoised)", lambda: ctx.pa_noise_detect_dev(
                d_pool.data_ptr(), descs, sub, d_den.data_ptr() if write else None, W, d_var.data_ptr(), d_flat.data_ptr(), d_pic.data_ptr(), stream=stream),
                10, nbytes)
    # correctness of what was timed (FULL, with d_denoised), on the first and last picture
    torch.cuda.synchronize()
    for i in (0, N_PICS - 1):
        want = nu.detect(planes[i][0], 0)
        got = {"sb_var": d_var[i].cpu().numpy().view(np.uint64), "flat_noise": d_flat[i].cpu().numpy(), "picture": d_pic[i].cpu().numpy().view(np.uint32),
               "denoised": d_den[i].cpu().numpy()}
        assert all(np.array_equal(got[k], want[k]) for k in got), "the timed noise detection differs from the restatement"
        assert nu.arm(want["picture"]) == "whole_picture", "the probe's pictures must take the whole-picture arm"
    # the denoise entry uses d_denoised up, and a second call would filter filtered chroma: same work, other values; the times are what is wanted
    report("pa_denoise (class 3_1: luma copied back, Cb and Cr filtered)", lambda: ctx.pa_denoise_dev(
        d_pool.data_ptr(), descs, offsets, cstride, d_den.data_ptr(), W, d_flat.data_ptr(), d_pic.data_ptr(), stream=stream), 10, N_PICS * (2 * B["luma"] + 2 * B["luma"]))
    for write in (False, True):
        nbytes = N_PICS * (B["luma"] * (2 if write else 1) + B["tables"])
        src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")   # as in tools/pa_stats_probe.py; the copy moves every one of them twice
        dst = torch.zeros_like(src)
        report(f"yardstick: device-to-device copy of as many bytes as pa_noise_detect reads plus writes ({'with' if write else 'without'} d_denoised)",
               lambda: dst.copy_(src), 10, nbytes)
    # the download a host-side detector would cost (profiles/pa_stats_probe.jsonl has it for the same planes): pageable host memory, host clock
    dev = torch.zeros(N_PICS * B["planes"], dtype=torch.uint8, device="cuda:0")
    host = torch.zeros(N_PICS * B["planes"], dtype=torch.uint8)
    us = host_timed(lambda: (host.copy_(dev), torch.cuda.synchronize()), iters, torch.cuda.synchronize).median
    emit(lines, {"entry": f"yardstick: download of the planes of {N_PICS} picture(s) to pageable host memory", "kind": "host clock around synchronous copies",
                 "pictures": N_PICS, "us": round(us, 1), "bytes": N_PICS * B["planes"], "GB_per_s": round(N_PICS * B["planes"] / us / 1e3, 1),
                 "detection_only_sub_us": round(detect_us[(1, False)], 1), "cheaper_than_the_download": detect_us[(1, False)] < us})
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 7, cpu=True, resources=True)
    a = ap.parse_args()
    lines = []
    if a.resources:
        return resources("pa_noise.hip", a.resources)
    if a.cpu:
        cpu_yardstick(lines)
    else:
        device_times(lines, a.iters)
    write_rows(a.out, lines)


if __name__ == "__main__":
    main()
