"""Flush time of the batcher's RD transform-type search against the same candidates flushed through plain _add.

Workload: bench.py's tu_batcher leg -- per superblock 1 x 64x64 (DCT_DCT), 4 x 32x32 (DCT_DCT, IDTX), 16 x 16x16, 64 x 8x8 and 256 x 4x4
(DCT_DCT, ADST_ADST, IDTX each): 1 017 candidates per superblock, i.e. 1 / 8 / 48 / 192 / 768 candidates of the five sizes.  As search
TUs that is 341 TUs per superblock whose type masks give exactly those candidates; the search flush adds the rate kernel (one launch
per size) and the decision kernel and downloads one record per TU.  Adds are not timed (the Python ctypes loop would dominate).

    python tools/tx_search_probe.py [--sbs 1,30,510] [--reps N] [--out FILE]

Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/tx_search_probe.py --sbs 510` (a separate run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "svt-av1-1_amd", "python")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sbs", default="1,30,510")
    ap.add_argument("--reps", type=int, default=0, help="timed flushes per point (default: 6 / 3 / 1 by size)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import svtav1_hip
    dev = "cuda:0"
    z = np.load(os.path.join(ROOT, "tests", "golden", "quant_tables.npz"))
    g = np.load(os.path.join(ROOT, "tests", "golden", "coeff_rate.npz"))
    qrows = np.ascontiguousarray(z["rows_bd8_inter"][[20, 120, 200], 0, :])
    d_qp = torch.from_numpy(qrows).to(dev)
    d_iscan = torch.from_numpy(z["iscan_pool"]).to(dev)
    d_tables = torch.from_numpy(np.ascontiguousarray(g["tables"][1])).to(dev)
    offs = [[int(z["scan_offsets"][int(z["scan_index"][ts, t])]) for t in range(16)] for ts in range(19)]
    pic_w, pic_h = 1920, 1088
    rng = torch.Generator().manual_seed(1)
    src = torch.randint(0, 256, (pic_w * pic_h,), dtype=torch.uint8, generator=rng).to(dev)
    pred = (src.short() + torch.randint(-6, 7, src.shape, dtype=torch.int16, generator=rng).to(dev)).clamp_(0, 255).to(torch.uint8)
    tus = []   # (tx_size, mask, x, y)
    for n, types in ((64, (0,)), (32, (0, 9)), (16, (0, 3, 9)), (8, (0, 3, 9)), (4, (0, 3, 9))):
        ts = svtav1_hip.TX_SIZES_WH.index((n, n))
        for y in range(0, 64, n):
            for x in range(0, 64, n):
                tus.append((ts, sum(1 << t for t in types), x, y))
    cand_per_sb = sum(bin(m).count("1") for _, m, _, _ in tus)
    coeff_per_sb = sum(min(svtav1_hip.TX_SIZES_WH[ts][0], 32) ** 2 * bin(m).count("1") for ts, m, _, _ in tus)
    ctx = svtav1_hip.Context(0)
    out = {"candidates_per_superblock": cand_per_sb, "search_tus_per_superblock": len(tus), "device": torch.cuda.get_device_name(0)}
    for G in [int(s) for s in a.sbs.split(",")]:
        reps = a.reps or (1 if G >= 510 else 3 if G >= 30 else 6)
        row = {}
        for mode in ("add", "search"):
            b = svtav1_hip.TuBatcher(ctx, G * cand_per_sb, G * coeff_per_sb)
            times = []
            for r in range(reps + 1):
                b.begin(src.data_ptr(), pred.data_ptr(), None, 0, d_qp.data_ptr(), d_iscan.data_ptr())
                if mode == "search":
                    b.set_tx_search(d_tables.data_ptr(), offs)
                for gi in range(G):
                    ox, oy = (gi % 30) * 64, (gi // 30) * 64
                    for ts, m, x, y in tus:
                        off = (oy + y) * pic_w + ox + x
                        if mode == "search":
                            b.add_tx_search(lambda_=60000, src_offset=off, src_stride=pic_w, pred_offset=off, pred_stride=pic_w, qparam_index=gi % 3,
                                            type_mask=m, tx_size=ts, is_inter=1, txb_skip_ctx=gi % 13, dc_sign_ctx=gi % 3)
                        else:
                            for t in range(16):
                                if m >> t & 1:
                                    b.add(ts, t, off, pic_w, off, pic_w, svtav1_hip.TU_RECON_SCRATCH, 0, gi % 3, offs[ts][t])
                ctx.synchronize()
                t0 = time.perf_counter()
                b.flush()
                dt = time.perf_counter() - t0
                if r:   # the first flush of a batcher warms up (code objects, pinned pages)
                    times.append(dt)
            b.close()
            row[f"{mode}_ms_per_flush"] = round(float(np.median(times)) * 1e3, 4)
        row["search_over_add"] = round(row["search_ms_per_flush"] / row["add_ms_per_flush"], 3)
        out[f"flush_per_{G}_sb"] = row
        print(G, row, flush=True)
    ctx.close()
    js = json.dumps(out, indent=1)
    print(js)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(js + "\n")


if __name__ == "__main__":
    main()
