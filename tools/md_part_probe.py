#!/usr/bin/env python3
"""Times mode decision's partition decision for one 1920 x 1080 picture, with 64x64 (510) and 128x128 (135) superblocks and with the
all-blocks list (forward_all_blocks_to_md) and the squares-only list (forward_sq_blocks_to_md) of an inter slice:
  * svthip_md_partition_batch_dev alone, next to the host round trip it replaces, measured in the same run on the same arrays: the
    decision array to pinned host memory, a stream synchronise, the per-block records and the final lists (with their counts) uploaded from
    pinned memory, a synchronise -- and NO host computation in between;
  * svthip_md_partition_compose_dev, next to a device-to-device copy of the three planes of the picture;
  * svthip_md_partition_picture_dev, next to the sum of its two parts.

    python tools/md_part_probe.py [--iters N] [--out FILE] [--tag TEXT]      device times (needs a GPU)
    python tools/md_part_probe.py --resources FILE                           registers, LDS and scratch of the kernels from the compiler's remarks

The tile pool holds the winner tile of a block at its picture position in the layer of its shape (nine pictures stacked), so blocks of
different depths share tiles: the composition reads the same bytes a real pool would give it.  Device times are microseconds per call: the
median, minimum and maximum over N samples, each the mean of back-to-back calls queued behind a sleep kernel, as tools/probe_common.py: timed
takes them.  What was timed is compared with the restatement (tests/md_part_util.py) on a sample of the superblocks before it is
reported.  One JSON line per row, appended to --out.  No threshold is set here."""
import argparse
import functools

import numpy as np

from probe_common import add_common_args, as_dev, emit, host_timed, open_stream, resources, timed, write_rows  # sets the import path

import svtav1_hip  # noqa: E402

W, H = 1920, 1080
LAYER_H = 1088


def build(sb_size, kind, rng, pu):
    """the arrays of one call: every superblock of the picture with the list of `kind`, costs of area times 95..105"""
    g = pu.geometry(sb_size)
    origins = pu.sb_origins(W, H, sb_size)
    lists, by_pattern = [], {}
    for ox, oy in origins:
        ins = pu.inside(sb_size, ox, oy, W, H)
        key = ins.tobytes()
        if key not in by_pattern:
            by_pattern[key] = np.array(pu.leaf_list(kind, sb_size, ins, False), np.int64).reshape(-1, 3)
        lists.append(by_pattern[key])
    n_leaf = sum(len(x) for x in lists)
    sbs, leaves = np.zeros(len(origins), pu.SB_DTYPE), np.zeros(n_leaf, pu.LEAF_DTYPE)
    at = 0
    for k, ((ox, oy), ls) in enumerate(zip(origins, lists)):
        sbs[k] = (at, len(ls), 60 + k % 50, ox, oy)
        m = ls[:, 0]
        part = leaves[at:at + len(ls)]
        part["mds_idx"], part["tot_d1_blocks"], part["split_flag"] = m, ls[:, 1], ls[:, 2]
        gx, gy, shape = (g[k][m].astype(np.int64) for k in ("origin_x", "origin_y", "shape"))
        part["pool_x"], part["pool_y"] = ox + gx, shape * LAYER_H + oy + gy
        at += len(ls)
    leaves["decision_index"] = np.arange(n_leaf)
    decisions = np.zeros(n_leaf, pu.DECISION_DTYPE)
    area = g["bwidth"].astype(np.int64) * g["bheight"]
    decisions["cost"] = area[leaves["mds_idx"]] * rng.integers(95, 106, n_leaf)
    return origins, lists, sbs, leaves, decisions


def device_times(lines, iters, tag=None):
    import torch

    import md_part_util as pu
    ctx = svtav1_hip.Context(0)
    torch_stream, stream = open_stream(torch)
    upload = functools.partial(as_dev, torch)
    rng = np.random.default_rng(3)
    fac = rng.integers(150, 3000, (20, 11)).astype(np.int32)
    pool_h = 9 * LAYER_H
    pool = [rng.integers(0, 256, (pool_h, W), np.uint8), *(rng.integers(0, 256, (pool_h // 2, W // 2), np.uint8) for _ in range(2))]
    d_pool, d_dst = [upload(p) for p in pool], [torch.zeros(n, dtype=torch.uint8, device="cuda:0") for n in (W * H, W * H // 4, W * H // 4)]
    d_copy = [torch.zeros_like(t) for t in d_dst]
    planes = lambda ts, ys, cs: svtav1_hip.InterPlanes(ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ys, cs)  # noqa: E731
    pool_arg, dst_arg = planes(d_pool, W, W // 2), planes(d_dst, W, W // 2)

    def report(name, t, sb_size, kind, n_sb, n_leaf, how="device events", **more):
        row = {"entry": name, "kind": how, "width": W, "height": H, "sb_size": sb_size, "list": kind, "superblocks": n_sb, "leaves": n_leaf,
               "us": round(t.median, 1), "us_min": round(t.min, 1), "us_max": round(t.max, 1), **more}
        if tag:
            row["tag"] = tag
        emit(lines, row)

    for sb_size in (64, 128):
        n, max_final = len(pu.geometry(sb_size)), 1024 if sb_size == 128 else 256
        for kind in ("all", "sq"):
            origins, lists, sbs, leaves, decisions = build(sb_size, kind, rng, pu)
            n_sb, n_leaf = len(sbs), len(leaves)
            d_sb, d_leaf, d_dec = upload(sbs), upload(leaves), upload(decisions)
            d_result = torch.zeros(n_sb * n * 16, dtype=torch.uint8, device="cuda:0")
            d_final = torch.zeros(n_sb * max_final * 16, dtype=torch.uint8, device="cuda:0")
            d_count = torch.zeros(n_sb * 4, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            decide_args = (d_sb.data_ptr(), n_sb, d_leaf.data_ptr(), n_leaf, d_dec.data_ptr(), n_leaf, sb_size, 0, fac, d_result.data_ptr(), d_final.data_ptr(),
                           d_count.data_ptr())
            compose_args = (pool_arg, W, pool_h, dst_arg, W, H)
            decide = lambda: ctx.md_partition_batch_dev(*decide_args, stream=stream)  # noqa: E731
            compose = lambda: ctx.md_partition_compose_dev(n_sb, d_leaf.data_ptr(), n_leaf, sb_size, d_final.data_ptr(), d_count.data_ptr(), *compose_args,  # noqa: E731
                                                           stream=stream)
            picture = lambda: ctx.md_partition_picture_dev(*decide_args, *compose_args, stream=stream)  # noqa: E731

            # what is about to be timed is right: a sample of superblocks against the restatement
            picture()
            torch_stream.synchronize()
            assert ctx.inter_pred_refused() == 0
            result = d_result.cpu().numpy().view(pu.RESULT_DTYPE).reshape(n_sb, n)
            final = d_final.cpu().numpy().view(pu.FINAL_DTYPE).reshape(n_sb, max_final)
            count = d_count.cpu().numpy().view(np.uint32)
            got = [t.cpu().numpy().reshape(s) for t, s in zip(d_dst, ((H, W), (H // 2, W // 2), (H // 2, W // 2)))]
            for k in sorted({0, 1, n_sb // 2, n_sb - 2, n_sb - 1}):
                first, ls = int(sbs["first_leaf"][k]), lists[k]
                r = pu.walk(sb_size, [tuple(x) for x in ls.tolist()], decisions["cost"][first:first + len(ls)].tolist(), int(sbs["full_lambda"][k]), fac, False)
                assert np.array_equal(result[k]["cost"], np.array(r["cost"], np.uint64)) and result[k]["part"].tolist() == r["part"], (sb_size, kind, k)
                assert final[k]["mds_idx"][:count[k]].tolist() == r["final"], (sb_size, kind, k)
                for f in final[k][:count[k]]:
                    x, y, w, h, lf = int(f["x"]), int(f["y"]), int(f["bwidth"]), int(f["bheight"]), leaves[int(f["leaf"])]
                    px, py = int(lf["pool_x"]), int(lf["pool_y"])
                    assert np.array_equal(got[0][y:y + h, x:x + w], pool[0][py:py + h, px:px + w]), (sb_size, kind, k, int(f["mds_idx"]))
            blocks = int(count.sum())

            t_decide, t_compose, t_picture = timed(torch, decide, iters), timed(torch, compose, iters), timed(torch, picture, iters)
            t_copy = timed(torch, lambda: [c.copy_(t) for c, t in zip(d_copy, d_dst)], iters)
            # the round trip the decision kernel replaces: host clock, pinned memory, no host computation
            h_dec = torch.empty(d_dec.numel(), dtype=torch.uint8).pin_memory()
            h_up = [torch.zeros(t.numel(), dtype=torch.uint8).pin_memory() for t in (d_result, d_final, d_count)]

            def round_trip():
                h_dec.copy_(d_dec, non_blocking=True)
                torch_stream.synchronize()
                for t, hst in zip((d_result, d_final, d_count), h_up):
                    t.copy_(hst, non_blocking=True)
                torch_stream.synchronize()

            t_trip = host_timed(round_trip, iters, torch_stream.synchronize)
            report("md_partition_batch_dev", t_decide, sb_size, kind, n_sb, n_leaf, final_blocks=blocks, over_round_trip=round(t_decide.median / t_trip.median, 2))
            report("yardstick: decisions to pinned host memory, synchronise, records and final lists uploaded, synchronise; no host computation", t_trip,
                   sb_size, kind, n_sb, n_leaf, how="host clock", bytes_down=int(d_dec.numel()), bytes_up=int(sum(t.numel() for t in h_up)))
            report("md_partition_compose_dev", t_compose, sb_size, kind, n_sb, n_leaf, final_blocks=blocks, over_plane_copy=round(t_compose.median / t_copy.median, 2))
            report("yardstick: device-to-device copy of the three planes", t_copy, sb_size, kind, n_sb, n_leaf, bytes=W * H * 3 // 2)
            report("md_partition_picture_dev", t_picture, sb_size, kind, n_sb, n_leaf, final_blocks=blocks,
                   over_its_parts=round(t_picture.median / (t_decide.median + t_compose.median), 2))
            del d_sb, d_leaf, d_dec, d_result, d_final, d_count
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 7, resources=True, tag=True)
    a = ap.parse_args()
    if a.resources:
        return resources("md_part.hip", a.resources, spill=True)
    lines = []
    device_times(lines, a.iters, a.tag)
    write_rows(a.out, lines)


if __name__ == "__main__":
    main()
