#!/usr/bin/env python3
"""Times film-grain Wiener denoising on one 1920 x 1080 and one 3840 x 2160 picture at 8 and at 10 bits:
svthip_[highbd_]film_grain_wiener_filter_dev (the four passes of the FFT filter), svthip_[highbd_]film_grain_dither_dev and the one-call
svthip_[highbd_]film_grain_wiener_denoise_dev, and next to them in the same run what the host path costs in transfers: the download of the
three source planes plus the upload of three denoised planes, pageable host memory.

    python tools/film_grain_denoise_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/film_grain_denoise_probe.py --cpu [--out FILE]                the CPU yardstick (build container only, where the reference exists)
    python tools/film_grain_denoise_probe.py --resources FILE                  registers, LDS and scratch of the kernels from the compiler's remarks

Device times are microseconds per call: the median over N samples of one call queued behind a sleep kernel, as tools/probe_common.py: timed
takes them.  --cpu times the reference's own aom_wiener_denoise_2d on one thread through the fixture driver
(tests/golden/ref_fg_denoise_driver.c): microseconds per picture, one call; it is measured on the build machine's CPU, not next to the
device.  Every denoise row carries the SHA-1 of the three denoised planes, device and reference alike: the rows of the two runs must
agree, which is the check of what was timed.  One JSON line per row, appended to --out.
For a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/film_grain_denoise_probe.py --iters 1"""
import argparse
import hashlib
import tempfile

import numpy as np

from probe_common import add_common_args, as_dev, emit, host_timed, open_stream, resources, timed, write_rows  # sets the import path

SIZES = ((1920, 1080), (3840, 2160))
BIT_DEPTHS = (8, 10)


def probe_picture(w, h, bd):
    import fg_model_util as mu
    return mu.make_planes(w, h, bd, np.random.default_rng([23, w, bd]))[0]


def planes_sha1(planes):
    return hashlib.sha1(b"".join(np.ascontiguousarray(p).tobytes() for p in planes)).hexdigest()


def cpu_yardstick(lines):
    import fg_denoise_util as du
    import make_golden_fg_denoise as gen
    assert gen.reference_available(), "the CPU yardstick needs the reference sources and oracle/_ref/obj_all"
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(tmp)
        for w, h in SIZES:
            for bd in BIT_DEPTHS:
                data = [np.ascontiguousarray(a) for a in probe_picture(w, h, bd)]
                den = [np.zeros_like(a) for a in data]
                psd = du.psd_of("default")
                t = L.drv_fgd_time(1, bd, w, h, *[a.ctypes.data for a in data], *[a.ctypes.data for a in den], *[a.shape[1] for a in data],
                                   *[a.ctypes.data for a in psd])
                emit(lines, {"entry": "reference aom_wiener_denoise_2d, 1 thread", "kind": "cpu, build container, host clock", "width": w, "height": h,
                             "bit_depth": bd, "us": round(t * 1e6, 1), "denoised_sha1": planes_sha1(den)})


def device_times(lines, iters):
    import torch

    import fg_denoise_util as du
    import svtav1_hip
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)

    def report(name, us, w, h, bd, kind="device events", **more):
        emit(lines, {"entry": name, "kind": kind, "width": w, "height": h, "bit_depth": bd, "us": round(us, 1), **more})

    for w, h in SIZES:
        for bd in BIT_DEPTHS:
            data = probe_picture(w, h, bd)
            dev = [as_dev(torch, a) for a in data]
            out = [torch.zeros_like(t) for t in dev]
            d_data, d_out, strides = [t.data_ptr() for t in dev], [t.data_ptr() for t in out], [w, w // 2, w // 2]
            psd_t = [as_dev(torch, a) for a in du.psd_of("default")]
            psd = [t.data_ptr() for t in psd_t]
            planes = torch.zeros(svtav1_hip.film_grain_wiener_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
            names = ("film_grain_wiener_filter_dev", "film_grain_dither_dev", "film_grain_wiener_denoise_dev")
            fns = [getattr(ctx, ("" if bd == 8 else "highbd_") + n) for n in names]
            filt = lambda: fns[0](d_data, strides, w, h, *(() if bd == 8 else (bd,)), psd, planes.data_ptr(), stream=stream)  # noqa: E731
            dith = lambda: fns[1](planes.data_ptr(), d_out, strides, w, h, *(() if bd == 8 else (bd,)), stream=stream)  # noqa: E731
            both = lambda: fns[2](d_data, strides, d_out, strides, w, h, *(() if bd == 8 else (bd,)), psd, stream=stream)  # noqa: E731
            nb = ((w + 31) // 32 + 1) * ((h + 31) // 32 + 1)
            report("film_grain_wiener_filter (four passes, three planes)", timed(torch, filt, iters, 1).median, w, h, bd, blocks=4 * 3 * nb)
            report("film_grain_dither (three planes)", timed(torch, dith, iters, 1).median, w, h, bd, dependent_steps=w + 2 * h)
            us = timed(torch, both, iters, 1).median
            torch.cuda.synchronize()
            report("film_grain_wiener_denoise, one call", us, w, h, bd, denoised_sha1=planes_sha1([t.cpu().numpy() for t in out]))
            host = [torch.zeros(t.numel(), dtype=torch.uint8) for t in dev]

            def transfers():
                for hst, t in zip(host, dev):
                    hst.copy_(t)
                for hst, t in zip(host, out):
                    t.copy_(hst)
                torch.cuda.synchronize()

            report("yardstick: download of three planes + upload of three denoised planes, pageable host memory",
                   host_timed(transfers, iters, torch.cuda.synchronize).median, w, h, bd, kind="host clock around synchronous copies",
                   bytes=2 * sum(t.numel() for t in dev))
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 3, cpu=True, resources=True)
    a = ap.parse_args()
    lines = []
    if a.resources:
        return resources("fg_denoise.hip", a.resources, spill=True)
    if a.cpu:
        cpu_yardstick(lines)
    else:
        device_times(lines, a.iters)
    write_rows(a.out, lines)


if __name__ == "__main__":
    main()
