#!/usr/bin/env python3
"""Times the five motion-analysis entries on synthetic 1920 x 1080 pictures (510 SBs each, 30 x 17, the last row 56 high: 480 complete), 1 and 12
pictures per launch, and next to them in the same run their yardsticks:
  for the two sample kernels (svthip_ma_zz_sad_dev, svthip_ma_ac_energy_dev) a device-to-device copy of as many bytes as the entry reads plus writes;
  for the three table kernels the download of the ME and OIS tables to pageable host memory plus a stream synchronise, what a host-side tail costs.

    python tools/ma_stats_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/ma_stats_probe.py --cpu [--out FILE]                the CPU yardstick (build container only, where the reference exists)

Device times are microseconds per LAUNCH: the median over N samples, each the mean of ten back-to-back calls queued behind a sleep kernel, as
tools/probe_common.py: timed takes them; min and max of the N samples are the run-to-run spread.  Bytes are what the algorithm reads and writes,
computed from the shapes.  The download is timed by the host clock around synchronous copies.  --cpu times the reference's own functions on one
picture, one thread, through the fixture driver (tests/golden/ref_ma_stats_driver.c, ASM_AVX2): microseconds per picture, best of five runs of 20
calls; the table group is MeBasedGlobalMotionDetection, DeriveSimilarCollocatedFlag, FailingMotionLcu and DetectUncoveredLcu (the histogram loop
is inline in the reference's thread body and not part of it).  One JSON line per row, appended to --out."""
import argparse
import functools
import json
import tempfile

import numpy as np

from probe_common import add_common_args, as_dev, emit, host_timed, open_stream, timed, write_rows  # sets the import path

W, H = 1920, 1080
COUNTS = (1, 12)


def picture(seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    luma = (128 + 60 * np.sin((x + 3 * seed) / 37.0) * np.cos((y - seed) / 23.0) + rng.integers(-6, 7, (H, W)) * ((x // 64 + y // 64) % 3 == 0)).clip(0, 255)
    return luma.astype(np.uint8)


def tables(rng, n_sb):
    """plausible ME rows and OIS words of one picture"""
    import ma_stats_util as mu
    me = np.zeros((n_sb, 85), mu.ME_DTYPE)
    me["xMvL0"], me["yMvL0"] = rng.integers(20, 30, (n_sb, 85)), rng.integers(-3, 4, (n_sb, 85))
    me["distortion"] = rng.integers(0, 30000, (n_sb, 85, 3))
    me["direction"], me["totalMeCandidateIndex"] = [0, 1, 2], 3
    cand = (rng.integers(0, 100000, (n_sb, 85, 18)).astype(np.uint32) | np.uint32(1 << 20))
    return me, cand


def cpu_yardstick(lines):
    import ma_stats_util as mu
    import make_golden_ma_stats as gen
    import pa_stats_util as pu
    assert gen.reference_available(), "the CPU yardstick needs the reference sources and oracle/_ref/obj_all"
    n_sb = mu.n_sbs(W, H)
    rng = np.random.default_rng(3)
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(tmp)
        cur, prev = picture(1), picture(0)
        y_mean, variance = pu.block_stats(cur, cur[::2, ::2], cur[::2, ::2], 0)[:2]
        me, cand = tables(rng, n_sb)
        item = {"me": me, "cand": cand, "y_mean": y_mean, "variance": variance, "ref_mean": y_mean[:, 0].copy(), "ref_var": variance[:, 0].copy(),
                "signals": np.array([0, 0, 3, 0, 0], np.int32)}
        assert L.drv_ma_open(W, H) == n_sb
        keep = [np.ascontiguousarray(a) for a in (cur, prev, y_mean)]
        out = [np.zeros(n_sb, np.uint32), np.zeros(n_sb, np.uint8), np.zeros(n_sb, np.uint8), np.zeros((n_sb, 5), np.uint64), np.zeros((n_sb, 5), np.uint64)]
        tb = [np.ascontiguousarray(item[k]) for k in ("me", "cand", "y_mean", "variance", "ref_mean", "ref_var", "signals")]
        gm, flags = np.zeros(6, np.int32), np.zeros((n_sb, 4), np.uint8)
        # every group is timed right after its own call: the groups share the picture control set (its slice type among the rest)
        calls = ((0, "ComputeDecimatedZzSad", lambda: L.drv_ma_zz(keep[0].ctypes.data, keep[1].ctypes.data, *[a.ctypes.data for a in out[:3]])),
                 (1, "CalculateAcEnergy (every SB of an intra picture)",
                  lambda: L.drv_ma_energy(keep[0].ctypes.data, 1, keep[2].ctypes.data, out[3].ctypes.data, out[4].ctypes.data)),
                 (2, "MeBasedGlobalMotionDetection + DeriveSimilarCollocatedFlag + FailingMotionLcu + DetectUncoveredLcu",
                  lambda: L.drv_ma_tables(*[a.ctypes.data for a in tb], gm.ctypes.data, flags.ctypes.data)))
        for which, name, call in calls:
            assert call() == 0
            t = min(L.drv_ma_time(which, 20) for _ in range(5)) / 20
            emit(lines, {"entry": f"reference {name}, 1 picture, 1 thread", "kind": "cpu, build container, host clock", "us": round(t * 1e6, 1)})
        L.drv_ma_close()


def device_times(lines, iters):
    import torch

    import ma_stats_util as mu
    import svtav1_hip
    from svtav1_hip import synth

    ctx = svtav1_hip.Context(0)
    torch_stream, stream = open_stream(torch)
    n_max, n_sb, complete = max(COUNTS), mu.n_sbs(W, H), int(mu.complete_sbs(W, H).sum())
    lumas = [picture(s) for s in range(n_max + 1)]
    pool, descs = svtav1_hip.build_picture_pool([synth.PaPicture(p) for p in lumas])
    d_pool = torch.from_numpy(pool).to("cuda:0")
    rng = np.random.default_rng(3)
    me, cand = zip(*[tables(rng, n_sb) for _ in range(n_max)])
    dev = functools.partial(as_dev, torch)
    d_me, d_cand = dev(np.stack(me)), dev(np.stack(cand))
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")  # noqa: E731
    d_y, d_v = dev(rng.integers(0, 256, (n_max + 1, n_sb, 85)).astype(np.uint8)), dev(rng.integers(0, 16000, (n_max + 1, n_sb, 85)).astype(np.uint16))
    d_sad, d_zz, d_nm = z((n_max, n_sb), torch.int32), z((n_max, n_sb), torch.uint8), z((n_max, n_sb), torch.uint8)
    d_energy, d_mean = z((n_max, n_sb, 5), torch.int64), z((n_max, n_sb, 5), torch.int64)
    d_rc, d_inter, d_intra = z((n_max, n_sb), torch.int32), z((n_max, n_sb), torch.int32), z((n_max, n_sb), torch.int32)
    d_hist, d_full, d_gm, d_flags = z((n_max, 2, 128), torch.int32), z((n_max,), torch.int32), z((n_max, 12), torch.int32), z((n_max, n_sb, 4), torch.uint8)
    torch.cuda.synchronize()

    def report(name, fn, n, nbytes=None, **more):
        us, lo, hi = timed(torch, fn, iters)
        row = {"entry": name, "kind": "device events", "pictures": n, "us": round(us, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), **more}
        if nbytes:
            row.update(bytes=nbytes, GB_per_s=round(nbytes / us / 1e3, 1))
        emit(lines, row)
        return us

    for n in COUNTS:
        cur, prev = descs[1:n + 1], descs[:n]
        intra = [svtav1_hip.make_ma_params(slice_is_intra=1)] * n
        inter = [svtav1_hip.make_ma_params(ref_index=j) for j in range(n)]
        zz_bytes, en_bytes = n * (complete * 512 + n_sb * 6), n * (complete * 4096 + n_sb * 5 + n_sb * 80)
        t_zz = report("ma_zz_sad", lambda: ctx.ma_zz_sad_dev(d_pool.data_ptr(), cur, prev, d_sad.data_ptr(), d_zz.data_ptr(), d_nm.data_ptr(), stream=stream), n, zz_bytes)
        t_en = report("ma_ac_energy (intra pictures)", lambda: ctx.ma_ac_energy_dev(d_pool.data_ptr(), cur, intra, d_y.data_ptr(), d_energy.data_ptr(),
                                                                                      d_mean.data_ptr(), stream=stream), n, en_bytes)
        for name, nbytes, t in (("ma_zz_sad", zz_bytes, t_zz), ("ma_ac_energy", en_bytes, t_en)):
            src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
            dst = torch.zeros_like(src)
            c = report(f"yardstick: device-to-device copy of the bytes {name} reads and writes", lambda: dst.copy_(src), n, nbytes)
            lines[-1]["entry_over_copy"] = round(t / c, 2)
            print(json.dumps({"entry_over_copy": lines[-1]["entry_over_copy"], "of": name, "pictures": n}), flush=True)
        t_tab = report("ma_distortion_stats", lambda: ctx.ma_distortion_stats_dev(d_me.data_ptr(), 85, d_cand.data_ptr(), W, H, inter, d_rc.data_ptr(), d_inter.data_ptr(),
                                                                                  d_intra.data_ptr(), d_hist.data_ptr(), d_full.data_ptr(), stream=stream), n)
        t_tab += report("ma_global_motion", lambda: ctx.ma_global_motion_dev(d_me.data_ptr(), 85, W, H, inter, d_gm.data_ptr(), stream=stream), n)
        t_tab += report("ma_sb_flags", lambda: ctx.ma_sb_flags_dev(d_y.data_ptr() + n_sb * 85, d_v.data_ptr() + 2 * n_sb * 85, d_y.data_ptr(), d_v.data_ptr(), 85, n,
                                                                   d_me.data_ptr(), 85, d_cand.data_ptr(), W, H, inter, d_flags.data_ptr(), stream=stream), n)
        # what a host-side tail costs today: the ME and OIS tables to pageable host memory, and the synchronise
        nbytes = n * n_sb * 85 * (24 + 18 * 4)
        d_tab, h_tab = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0"), torch.zeros(nbytes, dtype=torch.uint8)
        us, lo, hi = host_timed(lambda: (h_tab.copy_(d_tab), torch_stream.synchronize()), iters, torch.cuda.synchronize)
        emit(lines, {"entry": "yardstick: download of the ME and OIS tables to pageable host memory and a stream synchronise", "kind": "host clock around synchronous copies",
                     "pictures": n, "us": round(us, 1), "us_min": round(lo, 1), "us_max": round(hi, 1), "bytes": nbytes,
                     "three_table_entries_us": round(t_tab, 2), "download_over_table_entries": round(us / t_tab, 1)})
    # correctness of what was timed last, on the first and last picture
    torch.cuda.synchronize()
    sad = d_sad.cpu().numpy().view(np.uint32)
    for i in (0, n_max - 1):
        assert np.array_equal(sad[i], mu.zz_sad(lumas[i + 1], lumas[i])[0]), "the timed ZZ SADs differ from the restatement"
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 9, cpu=True)
    a = ap.parse_args()
    lines = []
    if a.cpu:
        cpu_yardstick(lines)
    else:
        device_times(lines, a.iters)
    write_rows(a.out, lines)


if __name__ == "__main__":
    main()
