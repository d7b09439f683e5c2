#!/usr/bin/env python3
"""Times film-grain estimation on one 1920 x 1080 and one 3840 x 2160 picture at 8 and at 10 bits: svthip_[highbd_]film_grain_noise_model_dev
with a sparse flat-block map (a tenth of the blocks, scattered: what the top decile alone gives) and with an all-flat map,
svthip_[highbd_]film_grain_flat_block_features_dev with the tables given and in its one-call form, and next to them in the same run the
download of the six planes (data and denoised) to pageable host memory that a host-side aom_noise_model_update would cost.

    python tools/film_grain_model_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/film_grain_model_probe.py --cpu [--out FILE]                the CPU yardstick (build container only, where the reference exists)
    python tools/film_grain_model_probe.py --resources FILE                  registers, LDS and scratch of the kernels from the compiler's remarks

Device times are microseconds per call: the median over N samples of one call queued behind a sleep kernel, as tools/probe_common.py: timed
takes them.  The serial sums make the all-flat model call latency-bound: its time grows with the number of observed samples, not with the
bytes.  --cpu times the reference's own aom_noise_model_init + _update + _free and aom_flat_block_finder_run on one thread through the
fixture driver (tests/golden/ref_fg_model_driver.c): microseconds per picture, the better of two calls; it is measured on the build
machine's CPU, not next to the device.  Every model row carries the SHA-1 of the state, device and reference alike, and the status and
observation counts: the rows of the two runs must agree, which is the check of what was timed.  One JSON line per row, appended to --out.
For a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/film_grain_model_probe.py --iters 1"""
import argparse
import hashlib
import tempfile

import numpy as np

from probe_common import add_common_args, as_dev, emit, host_timed, open_stream, resources, timed, write_rows  # sets the import path

SIZES = ((1920, 1080), (3840, 2160))
BIT_DEPTHS = (8, 10)
MAPS = ("sparse", "all")


def probe_picture(w, h, bd):
    import fg_model_util as mu
    return mu.make_planes(w, h, bd, np.random.default_rng([23, w, bd]))


def probe_map(w, h, kind):
    import fg_model_util as mu
    nbw, nbh = mu.blocks_of(w, h)
    if kind == "all":
        return np.full((nbh, nbw), 255, np.uint8)
    return (np.random.default_rng([29, w]).random((nbh, nbw)) < 0.1).astype(np.uint8)


def state_row(state):
    return {"status": int(state["status"]), "observations": state["latest"]["num_observations"].tolist(),
            "equations": state["latest"]["strength_num_equations"].tolist(), "state_sha1": hashlib.sha1(state.tobytes()).hexdigest()}


def cpu_yardstick(lines):
    import fg_model_util as mu
    import make_golden_fg_model as gen
    assert gen.reference_available(), "the CPU yardstick needs the reference sources and oracle/_ref/obj_all"
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(tmp)
        for w, h in SIZES:
            for bd in BIT_DEPTHS:
                data, den = probe_picture(w, h, bd)
                _, _, args = keep = gen._plane_args(data, den)
                for kind in MAPS:
                    flat = probe_map(w, h, kind)
                    t = min(L.drv_fgm_time(0, 1, bd, w, h, *args, flat.ctypes.data) for _ in range(2))
                    emit(lines, {"entry": f"reference aom_noise_model_init + _update, {kind} map, 1 thread", "kind": "cpu, build container, host clock",
                                 "width": w, "height": h, "bit_depth": bd, "flat_blocks": int(np.count_nonzero(flat)), "us": round(t * 1e6, 1),
                                 **state_row(gen.reference_state(L, bd, data, den, flat))})
                t = min(L.drv_fgm_time(1, 1, bd, w, h, *args, None) for _ in range(2))
                final = gen.reference_final_map(L, bd, data[0])
                emit(lines, {"entry": "reference aom_flat_block_finder_run, 1 thread", "kind": "cpu, build container, host clock", "width": w, "height": h,
                             "bit_depth": bd, "us": round(t * 1e6, 1), "final_map_sha1": hashlib.sha1(final.tobytes()).hexdigest()})
                del keep


def device_times(lines, iters):
    import torch

    import fg_model_util as mu
    import svtav1_hip
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)

    def report(name, us, w, h, bd, kind="device events", **more):
        emit(lines, {"entry": name, "kind": kind, "width": w, "height": h, "bit_depth": bd, "us": round(us, 1), **more})

    for w, h in SIZES:
        nb = int(np.prod(mu.blocks_of(w, h)))
        for bd in BIT_DEPTHS:
            data, den = probe_picture(w, h, bd)
            dev = [as_dev(torch, a) for a in (*data, *den)]
            d_data, d_den, strides = [t.data_ptr() for t in dev[:3]], [t.data_ptr() for t in dev[3:]], [w, w // 2, w // 2]
            d_state = torch.zeros(mu.STATE.itemsize, dtype=torch.uint8, device="cuda:0")
            d_feat = torch.zeros(nb * mu.FEATURES.itemsize, dtype=torch.uint8, device="cuda:0")
            d_is = torch.zeros(nb, dtype=torch.uint8, device="cuda:0")
            d_tab = torch.zeros(mu.TABLES_DOUBLES, dtype=torch.float64, device="cuda:0")
            for kind in MAPS:
                flat = probe_map(w, h, kind)
                d_flat = as_dev(torch, flat)
                model = (lambda: ctx.film_grain_noise_model_dev(d_data, d_den, strides, w, h, d_flat.data_ptr(), d_state.data_ptr(), stream=stream)) if bd == 8 \
                    else (lambda: ctx.highbd_film_grain_noise_model_dev(d_data, d_den, strides, w, h, bd, d_flat.data_ptr(), d_state.data_ptr(), stream=stream))
                us = timed(torch, model, iters, 1).median
                torch.cuda.synchronize()
                state = np.frombuffer(d_state.cpu().numpy().tobytes(), mu.STATE)[0]
                report(f"film_grain_noise_model, {kind} map", us, w, h, bd, flat_blocks=int(np.count_nonzero(flat)), **state_row(state))
            ctx.film_grain_flat_block_tables_dev(d_tab.data_ptr(), stream=stream)
            feats = (lambda tab: ctx.film_grain_flat_block_features_dev(d_data[0], w, w, h, d_feat.data_ptr(), d_is.data_ptr(), tab, stream=stream)) if bd == 8 \
                else (lambda tab: ctx.highbd_film_grain_flat_block_features_dev(d_data[0], w, w, h, bd, d_feat.data_ptr(), d_is.data_ptr(), tab, stream=stream))
            report("film_grain_flat_block_features, tables given", timed(torch, lambda: feats(d_tab.data_ptr()), iters, 4).median, w, h, bd, blocks=nb)
            report("film_grain_flat_block_features, one call (tables + features)", timed(torch, lambda: feats(None), iters, 4).median, w, h, bd, blocks=nb)
            torch.cuda.synchronize()
            final, _, _ = mu.finish_flat_blocks(np.frombuffer(d_feat.cpu().numpy().tobytes(), mu.FEATURES), d_is.cpu().numpy())
            report("film_grain_flat_block_tables", timed(torch, lambda: ctx.film_grain_flat_block_tables_dev(d_tab.data_ptr(), stream=stream), iters, 4).median,
                   w, h, bd, final_map_sha1=hashlib.sha1(final.tobytes()).hexdigest())
            host = [torch.zeros(t.numel(), dtype=torch.uint8) for t in dev]

            def download():
                for hst, t in zip(host, dev):
                    hst.copy_(t)
                torch.cuda.synchronize()

            report("yardstick: download of the six planes, pageable host memory", host_timed(download, iters, torch.cuda.synchronize).median, w, h, bd,
                   kind="host clock around synchronous copies", bytes=sum(t.numel() for t in dev))
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 3, cpu=True, resources=True)
    a = ap.parse_args()
    lines = []
    if a.resources:
        return resources("fg_noise_model.hip", a.resources, spill=True)
    if a.cpu:
        cpu_yardstick(lines)
    else:
        device_times(lines, a.iters)
    write_rows(a.out, lines)


if __name__ == "__main__":
    main()
