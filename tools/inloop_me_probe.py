#!/usr/bin/env python3
"""Times the in-loop motion estimation entries on one 1920 x 1080 picture: 510 superblocks, one list, a 64x64 area, centres (0, 0):
svthip_me_inloop_fullpel_search_dev with all 849 blocks and with the 640 blocks with a side of 4, and the one-call entry
svthip_me_inloop_search_dev (areas + full-pel search + reorder), svthip_me_inloop_subpel_search_dev on both block sets and the one-call entry with use_subpel.  On the
same superblocks and area, in the same run, the nearest existing kernels as the yardstick: svthip_me_fullpel_search209_dev and
svthip_me_subpel_search_dev(all_pu = 1, SUB_SAD_SEARCH).  The reference's times on one host thread are those the fixture generator
recorded (tests/golden/inloop_me.npz, ref_seconds_1080p, ref_seconds_1080p_subpel).

    python tools/inloop_me_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/inloop_me_probe.py --resources FILE                  registers, LDS and scratch of the kernels from the compiler's remarks

Device times are microseconds per launch: the median over N samples, each the mean of back-to-back calls queued behind a sleep kernel, as
tools/probe_common.py: timed takes them; the entries are sampled in alternation (one sample of each per round), so drift hits all alike.
`of_packed_sad_ceiling`: abs-diffs per second over the measured packed-SAD issue ceiling of DESIGN section 6 (1.56e14 abs-diff/s).  One
JSON line per row, printed and appended to --out (default profiles/inloop_me_probe.jsonl) once the run has finished.
The resource report comes from the hipcc line of tools/probe_common.py: resources (gfx950, -O3, -fPIC, -std=c++17, the compiler's
resource-usage remarks) on csrc/me_inloop.hip.  Its LDS size of 0 is right: the kernels' LDS is dynamic (inloop_lds_bytes), 24 300 bytes
for a 64x64 area and 44 776 for 127x127."""
import argparse
import functools
import json
import os

import numpy as np

from probe_common import ROOT, add_common_args, as_dev, open_stream, resources, timed, write_rows  # sets the import path

PACKED_SAD_CEILING = 1.56e14   # abs-diff/s, DESIGN section 6
W, H, AREA = 1920, 1080, 64


def device_times(iters, out):
    import torch

    import me_inloop_util as iu
    import svtav1_hip
    from svtav1_hip import synth
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    dev = functools.partial(as_dev, torch)
    cur, ref = synth.PaPicture(synth.synth_luma(W, H, 1)), synth.PaPicture(synth.synth_luma(W, H, 0))
    sbs = iu.sb_origins(W, H)
    n = len(sbs)
    assert n == 510
    S, PAD = cur.stride, synth.PAD_FULL
    geom = (S, PAD, PAD)
    d_src, d_ref = dev(cur.full), dev(ref.full)
    d_sb, d_center = dev(sbs.astype(np.uint16)), dev(np.zeros((n, 2), np.int16))
    d_desc = torch.zeros(n * 8, dtype=torch.int32, device="cuda:0")
    d_sad, d_mv = (torch.zeros(n * iu.N_BLOCKS, dtype=torch.int32, device="cuda:0") for _ in range(2))
    d_out = torch.zeros(n * iu.N_BLOCKS * 2, dtype=torch.int16, device="cuda:0")
    ctx.reserve(W, H, svtav1_hip.INLOOP_ME_PU_COUNT)
    ctx.inloop_area_dev(d_center.data_ptr(), d_sb.data_ptr(), n, W, H, geom, geom, AREA, AREA, d_desc.data_ptr(), stream=stream)
    # the yardstick's descriptors: the open-loop search's own window rules on the same centres
    desc209 = svtav1_hip.make_fullpel_desc(cur, ref, None, AREA, AREA)
    d_desc209 = dev(desc209)
    d_sad209, d_mv209 = (torch.zeros(n * 209, dtype=torch.int32, device="cuda:0") for _ in range(2))
    d_sad2, d_mv2 = (torch.zeros(n * iu.N_BLOCKS, dtype=torch.int32, device="cuda:0") for _ in range(2))   # what the refinement works on
    d_out2 = torch.zeros(n * iu.N_BLOCKS * 2, dtype=torch.int16, device="cuda:0")
    A = lambda t: t.data_ptr()  # noqa: E731
    ctx.inloop_fullpel_search_dev(A(d_src), S, A(d_ref), S, A(d_desc), n, svtav1_hip.INLOOP_BLOCKS_ALL, A(d_sad2), A(d_mv2), stream=stream)
    entries = [
        ("inloop full-pel, all 849 blocks", lambda: ctx.inloop_fullpel_search_dev(A(d_src), S, A(d_ref), S, A(d_desc), n, svtav1_hip.INLOOP_BLOCKS_ALL, A(d_sad), A(d_mv),
                                                                                  stream=stream)),
        ("inloop full-pel, the 640 blocks with a side of 4", lambda: ctx.inloop_fullpel_search_dev(A(d_src), S, A(d_ref), S, A(d_desc), n,
                                                                                                    svtav1_hip.INLOOP_BLOCKS_SIDE_4, A(d_sad), A(d_mv), stream=stream)),
        ("inloop one-call entry (areas, full-pel all blocks, reorder)", lambda: ctx.inloop_search_dev(A(d_src), geom, A(d_ref), geom, W, H, A(d_center), A(d_sb), n, AREA,
                                                                                                       AREA, A(d_sad), A(d_mv), A(d_out), stream=stream)),
        ("inloop sub-pel refinement, all blocks (713 refined)", lambda: ctx.inloop_subpel_search_dev(A(d_src), S, A(d_ref), S, A(d_desc), n, svtav1_hip.INLOOP_BLOCKS_ALL,
                                                                                                      A(d_sad2), A(d_mv2), stream=stream)),
        ("inloop sub-pel refinement, the blocks with a side of 4 (512 refined)", lambda: ctx.inloop_subpel_search_dev(
            A(d_src), S, A(d_ref), S, A(d_desc), n, svtav1_hip.INLOOP_BLOCKS_SIDE_4, A(d_sad2), A(d_mv2), stream=stream)),
        ("inloop one-call entry with use_subpel (areas, full-pel, refinement, reorder)", lambda: ctx.inloop_search_dev(
            A(d_src), geom, A(d_ref), geom, W, H, A(d_center), A(d_sb), n, AREA, AREA, A(d_sad2), A(d_mv2), A(d_out2), use_subpel=True, stream=stream)),
        ("yardstick: svthip_me_fullpel_search209_dev", lambda: ctx.fullpel_search209_dev(A(d_src), S, A(d_ref), S, A(d_desc209), n, AREA, AREA, A(d_sad209), A(d_mv209),
                                                                                         stream=stream)),
        ("yardstick: svthip_me_subpel_search_dev(all_pu = 1, SUB_SAD_SEARCH)", lambda: ctx.subpel_search_dev(
            A(d_src), S, A(d_ref), S, A(d_desc209), n, AREA, AREA, A(d_sad209), A(d_mv209), svtav1_hip.FRACTIONAL_SUB_SAD_SEARCH, True, stream=stream)),
    ]
    torch.cuda.synchronize()
    samples = {name: [] for name, _ in entries}
    for _ in range(iters):            # alternating: one sample of every entry per round
        for name, fn in entries:
            samples[name].append(timed(torch, fn, 1, 4).median)
    # correctness of what was timed: the one-call entry ran last on d_sad / d_mv / d_out
    torch.cuda.synchronize()
    desc = d_desc.cpu().numpy().reshape(n, 8)
    want = iu.area(np.zeros((n, 2), np.int16), sbs, W, H, geom, geom, AREA, AREA)
    assert np.array_equal(desc, want), "timed search areas differ"
    check = [0, 29, 255, 509]         # a corner, the 56-row bottom edge, the interior
    sad, mv = iu.fullpel(cur.full.reshape(-1), S, ref.full.reshape(-1), S, want[check])
    got_sad, got_mv = d_sad.cpu().numpy().view(np.uint32).reshape(n, -1)[check], d_mv.cpu().numpy().view(np.uint32).reshape(n, -1)[check]
    assert np.array_equal(got_sad, sad) and np.array_equal(got_mv, mv), "timed full-pel search differs"
    assert np.array_equal(d_out.cpu().numpy().reshape(n, iu.N_BLOCKS, 2)[check], iu.pack(mv)), "timed reorder differs"
    # the one-call entry with use_subpel ran last on d_sad2 / d_mv2 / d_out2
    sub_sad, sub_mv = iu.subpel(cur.full.reshape(-1), S, ref.full.reshape(-1), S, want[check], sad, mv)
    got_sad, got_mv = d_sad2.cpu().numpy().view(np.uint32).reshape(n, -1)[check], d_mv2.cpu().numpy().view(np.uint32).reshape(n, -1)[check]
    assert np.array_equal(got_sad, sub_sad) and np.array_equal(got_mv, sub_mv), "timed sub-pel refinement differs"
    assert np.array_equal(d_out2.cpu().numpy().reshape(n, iu.N_BLOCKS, 2)[check], iu.pack(sub_mv)), "timed reorder after the refinement differs"
    positions = int((want[:, 4] * want[:, 5]).sum())
    absdiff = positions * 4096
    med = {name: float(np.median(v)) for name, v in samples.items()}
    base209 = med["yardstick: svthip_me_fullpel_search209_dev"]
    lines = []
    for name, _ in entries:
        row = {"entry": name, "kind": "device events, median of alternating samples", "width": W, "height": H, "superblocks": n, "area": [AREA, AREA],
               "us": round(med[name], 1), "samples": iters}
        if name.startswith("inloop sub-pel"):
            row.update({"ratio_to_subpel_search_all_pu_sub_sad": round(med[name] / med["yardstick: svthip_me_subpel_search_dev(all_pu = 1, SUB_SAD_SEARCH)"], 2)})
        elif name.startswith("inloop"):
            row.update({"positions": positions, "ratio_to_fullpel209": round(med[name] / base209, 2),
                        "of_packed_sad_ceiling": round(absdiff / (med[name] * 1e-6) / PACKED_SAD_CEILING, 3)})
        lines.append(row)
    fx = iu.load_fixture()
    ref_s = float(fx["ref_seconds_1080p"])
    lines.append({"entry": "reference in_loop_motion_estimation_sblock, one host thread, use_subpel_flag = 0 (from the fixture generator)", "kind": "host clock",
                  "width": W, "height": H, "superblocks": n, "area": [AREA, AREA], "us": round(ref_s * 1e6, 0),
                  "ratio_to_inloop_full_pel_all": round(ref_s * 1e6 / med["inloop full-pel, all 849 blocks"], 0)})
    sub_s = float(fx["ref_seconds_1080p_subpel"])
    lines.append({"entry": "reference in_loop_motion_estimation_sblock, one host thread, use_subpel_flag = 1 (from the fixture generator)", "kind": "host clock",
                  "width": W, "height": H, "superblocks": n, "area": [AREA, AREA], "us": round(sub_s * 1e6, 0)})
    for row in lines:
        print(json.dumps(row), flush=True)
    write_rows(out, lines)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 9, out_default=os.path.join(ROOT, "profiles", "inloop_me_probe.jsonl"), resources=True)
    a = ap.parse_args()
    if a.resources:
        resources("me_inloop.hip", a.resources, spill=True)
    else:
        device_times(a.iters, a.out)


if __name__ == "__main__":
    main()
