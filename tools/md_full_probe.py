#!/usr/bin/env python3
"""Times mode decision's full loop for one 1920 x 1080 picture at three luma sizes, 8x8, 32x32 and 64x64, each with has_uv, four candidates
a block and all four picked (max_full 4): svthip_md_full_loop_batch_dev, the whole call with every stage, once without a tx-type search
(both masks 1) and once with the ENC_M1 masks; and at 128x128 (svthip_md_full_loop128_batch_dev: four luma TUs of 64x64 and four chroma TUs
of 32x32 a plane and slot, no search), whose 120 blocks of the 1920 x 1024 area hold the same 1 920 luma and 3 840 chroma TUs as the 480
blocks of the 64x64 row, so that the 64x64 row is its yardstick.  Next to it in the same run:
  * the launches the call is built around, alone, on the same TUs through the public entries -- svthip_encode_tu_batch_dev and
    svthip_coeff_rate_batch_dev on Y (every TxType of the search, then the winner's shape once more), Cb and Cr (as DCT_DCT) -- so that the difference
    is what the new kernels (expand, winner, cost, decide, copy) and the tx-type decision add;
  * the download, to pageable host memory, of the picks and of the per-slot eobs, distortion sums, energies and bits: what a host-side
    full loop on the same leaves costs before it adds up its first cost.

    python tools/md_full_probe.py [--iters N] [--out FILE] [--sizes 8,32,64,128] [--tag TEXT]      device times (needs a GPU)
    python tools/md_full_probe.py --resources FILE              registers, LDS and scratch of the kernels from the compiler's remarks

The prediction pool holds candidate c of the block at (x, y) at (x, c * 1080 + y): four pictures stacked; the slot pool has the same
shape.  Device times are microseconds per call: the median over N samples, each the mean of back-to-back calls queued behind a sleep
kernel, as tools/probe_common.py: timed takes them.  What was timed is compared with the restatement (tests/md_full_util.py) on a sample of
the blocks before it is reported.  One JSON line per row, appended to --out.  No threshold is set here."""
import argparse
import functools

import numpy as np

from probe_common import add_common_args, as_dev, emit, host_timed, open_stream, resources, timed, write_rows  # sets the import path

import svtav1_hip  # noqa: E402

W, H, SLOTS = 1920, 1080, 4
SIZES = (8, 32, 64, 128)
TU_MAX = 64   # a 128-wide block has TUs of 64x64 (chroma 32x32)


def build(size, search, rng, fu, mu):
    """the scenario of one size: every complete block of the picture is a group of four candidates, all picked"""
    nx, ny = W // size, H // size
    n_groups, n_cand = nx * ny, nx * ny * SLOTS
    s = fu.Scenario()
    s.name, s.w, s.h, s.n_groups, s.max_full, s.n_cand, s.reduced = f"{size}x{size}", size, size, n_groups, SLOTS, n_cand, 0
    s.cw, s.ch, s.tw, s.th = size // 2, size // 2, size, size
    s.mask_inter, s.mask_intra = fu.masks_of(size, size, search)
    yy, xx = np.mgrid[0:H, 0:W]
    luma = ((np.sin(xx / 17.0) + np.cos(yy / 11.0)) * 60 + 128 + rng.integers(-6, 7, (H, W))).clip(0, 255).astype(np.uint8)
    s.src = [luma, luma[::2, ::2].copy(), luma[1::2, 1::2].copy()]
    s.pool = [np.concatenate([(p.astype(np.int32) + rng.integers(-3 * (c + 1), 3 * (c + 1) + 1, p.shape)).clip(0, 255).astype(np.uint8)
                              for c in range(SLOTS)]) for p in s.src]
    fast, full = np.zeros((n_groups, SLOTS), fu.FAST_DTYPE), np.zeros((n_groups, SLOTS), fu.FULL_DTYPE)
    bx, by = (a.reshape(-1) for a in np.meshgrid(np.arange(nx) * size, np.arange(ny) * size))
    tu = min(size, TU_MAX)
    types_y, types_uv = svtav1_hip.valid_tx_types(tu, tu), svtav1_hip.valid_tx_types(tu // 2, tu // 2)
    for c in range(SLOTS):
        fast["src_x"][:, c], fast["src_y"][:, c], fast["pred_x"][:, c], fast["pred_y"][:, c] = bx, by, bx, by + c * H
        fast["flags"][:, c] = mu.TYPE_INTER if c & 1 else 0
        full["recon_x"][:, c], full["recon_y"][:, c] = bx, by
    fast["has_uv"], fast["lambda_"], fast["merge_rate"] = 1, 1500, mu.NO_MERGE
    full["luma_rate"], full["chroma_rate"] = rng.integers(50, 30000, full.shape), rng.integers(10, 9000, full.shape)
    full["skip_mode_rate"] = np.where((fast["flags"] & mu.TYPE_INTER != 0) & (rng.random(full.shape) < 0.5), rng.integers(20, 3000, full.shape), fu.NONE)
    full["lambda_"] = rng.integers(1000, 400000, full.shape)
    full["qparam_index"] = 3 * rng.integers(0, len(fu.QINDICES), full.shape)[..., None] + np.arange(3)
    full["tx_type_y"], full["tx_type_uv"] = np.asarray(types_y)[rng.integers(0, len(types_y), full.shape)], np.asarray(types_uv)[rng.integers(0, len(types_uv), full.shape)]
    full["txb_skip_ctx"], full["dc_sign_ctx"] = rng.integers(0, 13, full.shape + (3,)), rng.integers(0, 3, full.shape + (3,))
    full["intra_mode"] = rng.integers(0, 13, full.shape)
    s.fast, s.full = fast.reshape(-1), full.reshape(-1)
    s.groups = np.zeros(n_groups, fu.GROUP_DTYPE)
    s.groups["first"], s.groups["count"], s.groups["buffer_total_count"], s.groups["buffer_width"] = np.arange(n_groups) * SLOTS, SLOTS, SLOTS, 13
    s.picks = np.zeros(n_groups, fu.PICK_DTYPE)
    s.picks["best"], s.picks["buffer_cand"] = 0xFF, 0xFF
    order = np.argsort(~(fast["flags"][0] & mu.TYPE_INTER != 0), kind="stable")     # PreModeDecision puts the INTER candidates first
    s.picks["best"][:, :SLOTS], s.picks["buffer_cand"][:, :SLOTS], s.picks["full_count"], s.picks["disable_merge_index"] = order, np.arange(SLOTS), SLOTS, 1
    s.n_slots = n_groups * SLOTS
    return s


def sample_of(s, some, fu):
    """the groups `some` of s as a scenario of their own (same planes), for the restatement"""
    t = fu.Scenario()
    t.__dict__.update(s.__dict__)
    rows = (some[:, None] * SLOTS + np.arange(SLOTS)).reshape(-1)
    t.fast, t.full, t.picks = s.fast[rows].copy(), s.full[rows].copy(), s.picks[some].copy()
    t.groups = s.groups[some].copy()
    t.groups["first"] = np.arange(len(some)) * SLOTS
    t.n_groups, t.n_cand, t.n_slots = len(some), len(rows), len(rows)
    tiles = -(-len(rows) // fu.SLOT_TILES_PER_ROW)
    t.slot_shape = [(tiles * s.th, fu.SLOT_TILES_PER_ROW * s.tw)] + [(tiles * s.th // 2, fu.SLOT_TILES_PER_ROW * s.tw // 2)] * 2
    t.recon_shape = [p.shape for p in s.src]
    return t, rows


def device_times(lines, iters, sizes=SIZES, tag=None):
    import torch

    import md_fast_util as mu
    import md_full_util as fu
    from oracle.binding import Oracle
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)
    sh = fu.shared()
    upload = functools.partial(as_dev, torch)
    d_qp, d_iscan, d_tables = upload(sh["qparams"]), upload(sh["tabs"].iscan_pool), upload(sh["tables"])
    tiles_per_row = {size: W // size for size in SIZES}
    wide = None
    if 128 in sizes:
        import md_full128_util as wide

    def report(name, us, size, search, n_groups, kind="device events", **more):
        row = {"entry": name, "kind": kind, "width": W, "height": H, "block": f"{size}x{size}", "search": search, "groups": n_groups, "slots": n_groups * SLOTS,
               "us": round(us, 1), **more}
        if tag:
            row["tag"] = tag
        emit(lines, row)

    for size in sizes:
        for search in ("none", "m1"):
            if size > TU_MAX and search != "none":
                continue   # no search from 128 on
            rng = np.random.default_rng(size)
            s = build(size, "none" if size > TU_MAX else search, rng, fu, mu)
            if search == "m1" and (s.mask_inter | s.mask_intra) == 1:
                continue   # 64x64 has DCT_DCT alone: the same call
            n, cw = s.n_slots, size // 2
            tu_w, tu_cw, per_side = min(size, TU_MAX), min(size, TU_MAX) // 2, size // min(size, TU_MAX)
            n_tu = per_side * per_side                 # TUs a slot and plane
            d = {k: [torch.from_numpy(p).to("cuda:0") for p in planes] for k, planes in (("src", s.src), ("pool", s.pool))}
            d["slot"] = [torch.zeros((H * SLOTS // (2 if p else 1), W // (2 if p else 1)), dtype=torch.uint8, device="cuda:0") for p in range(3)]
            d["recon"] = [torch.zeros_like(t) for t in d["src"]]
            planes = {}
            for k, ts_ in d.items():
                a = svtav1_hip.InterPlanes()
                a.y, a.cb, a.cr = (t.data_ptr() for t in ts_)
                a.y_stride, a.c_stride = W, W // 2
                planes[k] = a
            d_fast, d_full, d_group, d_pick = upload(s.fast), upload(s.full), upload(s.groups), upload(s.picks)
            is_wide = size > TU_MAX
            work = svtav1_hip.md_full128_workspace_bytes(s.n_groups, SLOTS, size, size) if is_wide else \
                svtav1_hip.md_full_workspace_bytes(s.n_groups, SLOTS, size, size, s.mask_inter, s.mask_intra)
            d_work = torch.zeros(work, dtype=torch.uint8, device="cuda:0")
            d_result = torch.zeros(n * 144, dtype=torch.uint8, device="cuda:0")
            d_decision = torch.zeros(s.n_groups * 16, dtype=torch.uint8, device="cuda:0")

            d_tu_out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")

            def call(stages=fu.LUMA | fu.CHROMA | fu.DECIDE):
                if is_wide:
                    ctx.md_full_loop128_batch_dev(planes["src"], planes["pool"], d_fast.data_ptr(), d_full.data_ptr(), s.n_cand, d_group.data_ptr(),
                                                  d_pick.data_ptr(), s.n_groups, size, size, d_qp.data_ptr(), d_iscan.data_ptr(), sh["iscan_offsets"],
                                                  d_tables.data_ptr(), 0, SLOTS, planes["slot"], tiles_per_row[size], planes["recon"], d_work.data_ptr(), stages,
                                                  d_result.data_ptr(), d_tu_out.data_ptr(), d_decision.data_ptr(), stream=stream)
                    return
                ctx.md_full_loop_batch_dev(planes["src"], planes["pool"], d_fast.data_ptr(), d_full.data_ptr(), s.n_cand, d_group.data_ptr(), d_pick.data_ptr(),
                                           s.n_groups, size, size, d_qp.data_ptr(), d_iscan.data_ptr(), sh["iscan_offsets"], d_tables.data_ptr(), 0, s.mask_inter,
                                           s.mask_intra, SLOTS, planes["slot"], tiles_per_row[size], planes["recon"], d_work.data_ptr(), stages,
                                           d_result.data_ptr(), d_decision.data_ptr(), stream=stream)

            t_call = timed(torch, call, iters, 4).median
            t_stage = {name: timed(torch, lambda st=st: call(st), iters, 4).median for name, st in (("luma", fu.LUMA), ("chroma", fu.CHROMA), ("decide", fu.DECIDE))}
            # correctness of what was timed: a sample of the blocks against the restatement
            torch.cuda.synchronize()
            got_r, got_d = d_result.cpu().numpy().view(fu.RESULT_DTYPE), d_decision.cpu().numpy().view(fu.DECISION_DTYPE)
            some = np.arange(0, s.n_groups, max(1, s.n_groups // 24))
            sub, rows = sample_of(s, some, fu)
            if is_wide:
                sub.origins = wide.tu_origins(size, size)
                sub.slot_shape = [(-(-len(rows) // wide.SLOT_TILES_PER_ROW) * size // (2 if p else 1), wide.SLOT_TILES_PER_ROW * size // (2 if p else 1)) for p in range(3)]
                st = wide.full_loop(Oracle(), sub)
                assert np.array_equal(d_tu_out.cpu().numpy().view(wide.TU_DTYPE).reshape(-1, SLOTS)[some].reshape(-1), st["tu"]), "the timed per-TU records differ"
            else:
                st = fu.full_loop(Oracle(), sub)
            want_r = st["result"].copy()
            want_r["row"] = rows[want_r["row"]]
            assert np.array_equal(got_r.reshape(-1, SLOTS)[some].reshape(-1), want_r), "the timed result rows differ"
            for f in ("cost", "winner_slot", "winner_buffer", "best_intra_mode", "n_full"):
                assert np.array_equal(got_d[f][some], st["decision"][f]), f"the timed decisions differ ({f})"
            recon = [t.cpu().numpy() for t in d["recon"]]
            for g in some:
                x, y = int(s.full["recon_x"][g * SLOTS]), int(s.full["recon_y"][g * SLOTS])
                assert np.array_equal(recon[0][y:y + size, x:x + size], st["recon"][0][y:y + size, x:x + size]), "the timed reconstruction differs"
                assert np.array_equal(recon[1][y // 2:y // 2 + cw, x // 2:x // 2 + cw], st["recon"][1][y // 2:y // 2 + cw, x // 2:x // 2 + cw])
            assert ctx.inter_pred_refused() == 0

            # the launches alone, through the public entries, on the same TUs
            ts_y, ts_uv = fu.tx_size_of(tu_w, tu_w), fu.tx_size_of(tu_cw, tu_cw)
            both = s.mask_inter | s.mask_intra
            types = [t for t in range(16) if both >> t & 1] if both != 1 else []
            k = np.arange(n)
            tile_x, tile_y = (k % tiles_per_row[size]) * size, (k // tiles_per_row[size]) * size
            launches = []

            def add_launch(plane, w_, n_tu, tx, recon_plane, recon_off, recon_stride, want_dist, ts, tu_x=0, tu_y=0):
                """n_tu TUs of w_ x w_: slot by slot for a search's candidates (n_tu a multiple of the slots), TU by TU of a slot for a 128-wide
                block (tu_x, tu_y: each TU's luma offset inside its block)"""
                c = 1 if plane else 0
                slot = np.tile(np.arange(n), n_tu // n) if np.ndim(tu_x) == 0 else np.repeat(np.arange(n), n_tu // n)
                f = s.fast[slot // SLOTS * SLOTS + s.picks["best"][slot // SLOTS, slot % SLOTS]]
                r8 = (lambda v: v // 2) if plane else (lambda v: v)
                tu = np.zeros(n_tu, svtav1_hip.TU_DESC_DTYPE)
                stride = W // 2 if plane else W
                tu["src_offset"] = r8(f["src_y"].astype(np.int64) + tu_y) * stride + r8(f["src_x"].astype(np.int64) + tu_x)
                tu["pred_offset"] = r8(f["pred_y"].astype(np.int64) + tu_y) * stride + r8(f["pred_x"].astype(np.int64) + tu_x)
                tu["recon_offset"], tu["recon_stride"] = recon_off, recon_stride
                ncoef = min(w_, 32) ** 2
                tu["coeff_offset"], tu["iscan_offset"], tu["tx_type"] = np.arange(n_tu) * ncoef, sh["iscan_offsets"][ts][tx], tx
                tu["src_stride"] = tu["pred_stride"] = stride
                rd = np.zeros(n_tu, svtav1_hip.COEFF_RATE_DESC_DTYPE)
                rd["coeff_offset"], rd["iscan_offset"], rd["tx_type"], rd["plane_type"], rd["is_inter"] = tu["coeff_offset"], tu["iscan_offset"], tx, c, 1
                d_tu, d_rd = upload(tu), upload(rd)
                d_q = torch.zeros(n_tu * ncoef, dtype=torch.int32, device="cuda:0")
                d_eob = torch.zeros(n_tu, dtype=torch.int16, device="cuda:0")
                d_energy, d_dist = torch.zeros(n_tu, dtype=torch.int64, device="cuda:0"), torch.zeros(n_tu * 2, dtype=torch.int64, device="cuda:0")
                d_bits = torch.zeros(n_tu, dtype=torch.int32, device="cuda:0")
                keep = (d_tu, d_rd, d_q, d_eob, d_energy, d_dist, d_bits, recon_plane)
                src_p, pred_p = d["src"][plane].data_ptr(), d["pool"][plane].data_ptr()

                def go():
                    ctx.encode_tu_batch_dev(src_p, pred_p, recon_plane.data_ptr(), d_tu.data_ptr(), n_tu, w_, w_, d_qp.data_ptr(), d_iscan.data_ptr(), None,
                                            d_q.data_ptr(), None, d_eob.data_ptr(), d_energy.data_ptr() if want_dist else None,
                                            d_dist.data_ptr() if want_dist else None, stream=stream)
                    if want_dist:
                        ctx.coeff_rate_batch_dev(d_tables.data_ptr(), d_q.data_ptr(), d_eob.data_ptr(), d_iscan.data_ptr(), d_rd.data_ptr(), n_tu, ts,
                                                 d_bits.data_ptr(), stream=stream)
                launches.append((go, keep))

            slot_off = [tile_y * W + tile_x, (tile_y // 2) * (W // 2) + tile_x // 2]
            if is_wide:   # every TU of a plane in one launch, as the call has them
                t = np.tile(np.arange(n_tu), n)
                ox, oy = (t % per_side) * tu_w, (t // per_side) * tu_w
                off = [(np.repeat(tile_y, n_tu) + oy) * W + np.repeat(tile_x, n_tu) + ox, ((np.repeat(tile_y, n_tu) + oy) // 2) * (W // 2) + (np.repeat(tile_x, n_tu) + ox) // 2]
                add_launch(0, tu_w, n * n_tu, np.zeros(n * n_tu, np.int64), d["slot"][0], off[0], W, True, ts_y, ox, oy)
                for p in (1, 2):
                    add_launch(p, tu_cw, n * n_tu, np.zeros(n * n_tu, np.int64), d["slot"][p], off[1], W // 2, True, ts_uv, ox, oy)
            elif types:
                m = n * len(types)
                scratch = torch.zeros(m * size * size, dtype=torch.uint8, device="cuda:0")
                add_launch(0, size, m, np.repeat(types, n), scratch, np.arange(m) * size * size, size, True, ts_y)
                add_launch(0, size, n, np.zeros(n, np.int64), d["slot"][0], slot_off[0], W, False, ts_y)
            else:
                add_launch(0, size, n, s.full["tx_type_y"][k // SLOTS * SLOTS + s.picks["best"][k // SLOTS, k % SLOTS]], d["slot"][0], slot_off[0], W, True, ts_y)
            for p in (1, 2) if not is_wide else ():
                add_launch(p, cw, n, np.zeros(n, np.int64), d["slot"][p], slot_off[1], W // 2, True, ts_uv)
            t_leaves = timed(torch, lambda: [go() for go, _ in launches], iters, 4).median

            # what a host-side full loop downloads today: the picks and the per-slot eobs, sums, energies and bits
            per_slot = [torch.zeros(n * b, dtype=torch.uint8, device="cuda:0") for b in (3 * 2, 3 * 16, 8, 3 * 4)] + [d_pick]
            host = [torch.empty(t.shape, dtype=torch.uint8) for t in per_slot]
            t_down = host_timed(lambda: ([hst.copy_(t) for hst, t in zip(host, per_slot)], torch.cuda.synchronize()), iters, torch.cuda.synchronize).median
            tus = n * n_tu * 3 if is_wide else n * (len(types) + 1 if types else 1) + 2 * n
            report("md_full_loop128 (LUMA | CHROMA | DECIDE)" if is_wide else "md_full_loop (LUMA | CHROMA | DECIDE)", t_call, size, search, s.n_groups, tx_types=len(types) or 1, transform_units=tus, workspace_bytes=work,
                   call_over_leaves=round(t_call / t_leaves, 2), added_us=round(t_call - t_leaves, 1))
            for name, t in t_stage.items():
                report(f"md_full_loop, stage {name} alone", t, size, search, s.n_groups)
            report("the chain and rate launches alone (svthip_encode_tu_batch_dev, svthip_coeff_rate_batch_dev)", t_leaves, size, search, s.n_groups,
                   transform_units=tus)
            report("yardstick: download of the picks and the per-slot eobs, sums, energies and bits to pageable host memory", t_down, size, search, s.n_groups,
                   kind="host clock around synchronous copies", bytes=sum(t.numel() for t in per_slot))
            del d, d_work, launches, per_slot
            torch.cuda.empty_cache()
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 7, resources=True, tag=True)
    ap.add_argument("--sizes", default=",".join(str(v) for v in SIZES), help="luma sizes to time, of " + ", ".join(str(v) for v in SIZES))
    a = ap.parse_args()
    if a.resources:
        return resources("md_full.hip", a.resources, spill=True)
    lines = []
    sizes = tuple(int(v) for v in a.sizes.split(","))
    assert set(sizes) <= set(SIZES), sizes
    device_times(lines, a.iters, sizes, a.tag)
    write_rows(a.out, lines)


if __name__ == "__main__":
    main()
