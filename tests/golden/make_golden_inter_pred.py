"""Writes tests/golden/inter_pred.npz from the reference's own av1_inter_prediction / av1_inter_prediction_hbd
(tests/golden/ref_inter_pred_driver.c linked against the reference objects of the oracle build, oracle/_ref/obj_all).  Run in the build
container only, where the reference exists: the fixture is data and is what the GPU box checks.

    python tests/golden/make_golden_inter_pred.py

Contents (one picture size, PIC x PIC luma; the two padded reference pictures are not stored: reference_pictures(bd) computes them with
integer arithmetic, identically everywhere, and the tests call it)
  case_bw, case_bh, case_bd, case_start, case_count    one row per batch: luma size, bit depth, its PUs desc[start:start + count]
  desc                           INTER_PU_DESC_DTYPE rows of every batch (what the device entry takes)
  ref_frame_type                 per PU, the reference's ref_frame_type argument (desc.own_list is derived from it)
  pred_{y,cb,cr}_8 / _10         the prediction planes after the reference's calls (PIC x PIC / PIC/2 x PIC/2, filled with FILL first),
                                 uint8 / uint16, one per batch of that bit depth: batch i is row case_pred[i]
The cases cover the 22 sizes, the five sub-8x8 shapes with every intra / inter neighbour mix, uni list 0 / list 1 / BI, all 16 filter pairs,
vectors clamped on every edge, neighbours whose ref_frame[0] is not LAST_FRAME, 8 and 10 bits."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "svt-av1-1_amd", "python"), ROOT]

import inter_pred_util as ipu  # noqa: E402
import svtav1_hip  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

OUT = os.path.join(HERE, "inter_pred.npz")
PIC, BORDER = 128, 144
FILL = {8: 0x55, 10: 0x155}
INTRA, LAST, LAST2, BWDREF, ALTREF = 0, 1, 2, 5, 7


def build_driver(out_dir):
    """ref_inter_pred_driver.c by the recipe of oracle/ref_driver.py, with its signatures."""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_inter_pred_driver.c"), out_dir)
    L.drv_init.restype = C.c_int
    L.drv_own_list.restype = C.c_int
    L.drv_own_list.argtypes = [C.c_int]
    L.drv_predict.restype = C.c_int
    L.drv_predict.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.drv_init()
    return L


def reference_predict(L, refs, pred, desc, rft, bw, bh, bd):
    """The reference's calls for one batch: refs = (ref0, ref1) ipu.Picture, pred an ipu.Picture (updated in place)."""
    hbd = int(bd > 8)
    arrs = [refs[0].y, refs[0].cb, refs[0].cr, refs[1].y, refs[1].cb, refs[1].cr, pred.y, pred.cb, pred.cr]
    for a in arrs:
        assert a.flags.c_contiguous
    planes = (C.c_void_p * 9)(*[a.ctypes.data for a in arrs])
    strides = np.array([refs[0].y.shape[1], refs[0].cb.shape[1], refs[1].y.shape[1], refs[1].cb.shape[1], pred.y.shape[1], pred.cb.shape[1]],
                       np.int32)
    for d, rf in zip(desc, rft):
        x, y = int(d["pu_origin_x"]), int(d["pu_origin_y"])
        pu = np.array([x, y, d["dst_origin_x"], d["dst_origin_y"], bw, bh, ipu.SIZES.index((bw, bh)), d["interp_filters"], rf, d["pred_direction"],
                       d["mv"][0][0], d["mv"][0][1], d["mv"][1][0], d["mv"][1][1], d["mb_to_left_edge"], d["mb_to_right_edge"], d["mb_to_top_edge"],
                       d["mb_to_bottom_edge"], d["has_uv"]], np.int64).astype(np.int32)
        nb = np.zeros(9, np.int32)
        for k in range(3):
            # ref_frame[0] of the neighbour: intra, or an inter frame whose list the desc names (LAST for 0, BWDREF / LAST2 / ALTREF for 1)
            nb[3 * k] = INTRA if not d["nb_is_inter"][k] else (LAST if d["nb_list"][k] == 0 else (LAST2, BWDREF, ALTREF)[(x + y + k) % 3])
            nb[3 * k + 1], nb[3 * k + 2] = d["nb_mv"][k]
        assert L.drv_predict(hbd, bd, pu.ctypes.data, nb.ctypes.data, PIC, PIC, planes, strides.ctypes.data, refs[0].border, pred.border) == 0


def ref_frame_types(L, rng, desc):
    """a ref_frame_type per PU consistent with its direction, and desc.own_list from it (the reference's av1_set_ref_frame)"""
    rft = np.zeros(len(desc), np.int32)
    for i, d in enumerate(desc):
        if d["pred_direction"] == 0:
            rft[i] = int(rng.choice([LAST, LAST, LAST2]))      # LAST2 on list 0: its own piece takes list 1 in the reference
        elif d["pred_direction"] == 1:
            rft[i] = int(rng.choice([BWDREF, ALTREF]))
        else:
            rft[i] = 8 + int(rng.integers(0, 4))               # a compound ref_frame_type (>= TOTAL_REFS_PER_FRAME)
        d["own_list"] = L.drv_own_list(int(rft[i]))
    return rft


def make_cases(rng):
    """(bw, bh, bd, desc) batches"""
    cases = []
    for bd in (8, 10):
        for (bw, bh) in ipu.SIZES:
            # list 0, list 1 and BI below 2048 samples; one PU of the large sizes (their direction rotates over the sizes), which keeps
            # the fixture small -- the GPU tests cover every direction of every size against the restatement pinned here
            n = 3 if bw * bh < 2048 else 1
            desc = ipu.random_descs(rng, n, bw, bh, PIC, PIC, clamp_frac=0.3)
            if n == 1:
                desc["pred_direction"] = (bw + bh + bd) % 3
            cases.append((bw, bh, bd, desc))
        # every (filter_x, filter_y) pair on 8x8 (8-tap) and 4x16 (4-tap x, pieces)
        for (bw, bh) in ((8, 8), (4, 16)):
            desc = ipu.random_descs(rng, 16, bw, bh, PIC, PIC, clamp_frac=0.0)
            desc["interp_filters"] = [(f >> 2) << 16 | (f & 3) for f in range(16)]
            cases.append((bw, bh, bd, desc))
        # sub-8x8 shapes: every intra / inter mix of the neighbourhood, uni list 0 and list 1 (and BI where a neighbour is intra)
        for (bw, bh) in ipu.SUB8_SIZES:
            used = [k for k in range(3) if (k == 0 and bw == 4 and bh == 4) or (k == 1 and bh == 4) or (k == 2 and bw == 4)]
            mixes = [[(m >> j) & 1 for j in range(len(used))] for m in range(1 << len(used))]
            pos = []
            cols, rows = PIC // bw, PIC // bh
            cand = [(cx * bw, cy * bh) for cy in range(rows) for cx in range(cols) if ipu.geometry_has_uv(bw, bh, cx * bw, cy * bh)]
            order = rng.permutation(len(cand))
            dirs = []
            for mix in mixes:
                for direction in (0, 1, 2):
                    if direction == 2 and all(mix):
                        continue
                    pos.append(cand[order[len(pos)]])
                    dirs.append((mix, direction))
            desc = ipu.random_descs(rng, len(pos), bw, bh, PIC, PIC, clamp_frac=0.25, positions=pos)
            for i, (mix, direction) in enumerate(dirs):
                desc[i]["pred_direction"] = direction
                for j, k in enumerate(used):
                    desc[i]["nb_is_inter"][k] = mix[j]
            cases.append((bw, bh, bd, desc))
    return cases


def reference_pictures(bd):
    """The two reference pictures of the fixture, computed (not stored): integer arithmetic only, so every machine gets the same samples.
    Triangle waves of different periods per picture and plane (smooth areas and steep ramps), a two-bit integer-hash texture, and
    saturated / zero stripes so that both clips are reached; padded by BORDER luma / BORDER // 2 chroma samples (32 more columns on the right)."""
    vmax = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    out = []
    for t in range(2):
        planes = []
        for k, (pw, b) in enumerate(((PIC, BORDER), (PIC // 2, BORDER // 2), (PIC // 2, BORDER // 2))):
            h, w = pw + 2 * b, pw + 2 * b + 32
            yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
            period = 2 * vmax
            ramp = (xx * (5 + 2 * t + k) + yy * (3 + t) + (xx * yy >> (5 + k))) * (vmax + 1) // (48 + 16 * t) % period
            tri = np.where(ramp <= vmax, ramp, period - ramp)
            hsh = (xx * 0x9E3779B1 + yy * 0x85EBCA77 + (3 * t + k + 1) * 0xC2B2AE3D) & 0xFFFFFFFF
            hsh = ((hsh ^ (hsh >> 15)) * 0x2C1B3C6D) & 0xFFFFFFFF
            a = tri + ((hsh >> 13) & 3) * ((vmax + 1) >> 8) - ((vmax + 1) >> 8)
            a[(yy // 9 + xx // 13) % 11 == 0] = vmax
            a[(yy // 7 + xx // 5) % 13 == 0] = 0
            planes.append(np.clip(a, 0, vmax).astype(dt))
        out.append(ipu.Picture(*planes, BORDER))
    return out


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    rng = np.random.default_rng(20261016)
    cases = make_cases(rng)
    refs = {bd: reference_pictures(bd) for bd in (8, 10)}
    out = {}
    all_desc, all_rft, rows, py, pcb, pcr = [], [], [], [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        start = 0
        for (bw, bh, bd, desc) in cases:
            rft = ref_frame_types(L, rng, desc)
            dt = np.uint8 if bd == 8 else np.uint16
            pred = ipu.Picture(np.full((PIC, PIC), FILL[bd], dt), np.full((PIC // 2, PIC // 2), FILL[bd], dt),
                               np.full((PIC // 2, PIC // 2), FILL[bd], dt), 0)
            reference_predict(L, refs[bd], pred, desc, rft, bw, bh, bd)
            all_desc.append(desc)
            all_rft.append(rft)
            rows.append((bw, bh, bd, start, len(desc)))
            start += len(desc)
            py.append(pred.y)
            pcb.append(pred.cb)
            pcr.append(pred.cr)
    rows = np.array(rows, np.int32)
    out.update(case_bw=rows[:, 0], case_bh=rows[:, 1], case_bd=rows[:, 2], case_start=rows[:, 3], case_count=rows[:, 4],
               desc=np.concatenate(all_desc), ref_frame_type=np.concatenate(all_rft))
    for bd in (8, 10):   # predictions per bit depth, in the sample type of the planes (case_pred = row in those stacks)
        sel = [i for i in range(len(rows)) if rows[i, 2] == bd]
        out[f"pred_y_{bd}"], out[f"pred_cb_{bd}"], out[f"pred_cr_{bd}"] = (np.stack([a[i] for i in sel]) for a in (py, pcb, pcr))
    out["case_pred"] = np.array([sum(1 for j in range(i) if rows[j, 2] == rows[i, 2]) for i in range(len(rows))], np.int32)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(rows)} batches, {start} PUs, {os.path.getsize(OUT) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
