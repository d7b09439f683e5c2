"""CPU: the __device__ arithmetic of svt-av1-1_amd/csrc/md_full_kernels.h -- the expansion of the picks into slots and descriptors, the take-over
of the search's winner, the cost, the decision and the copy -- compiled for the host (tests/host_kernels/md_full_host.cpp behind
tests/host_kernels/hip_on_host.h) and run on the constructed cases of tests/md_full_util.py.  A stand-alone program with its own main, built
with -fsanitize=address,undefined.  The slot planes and the reconstructed picture are allocated to exactly their size, 0 and 3 bytes into
their allocations (the dword and the byte path of the copy), so a copy beyond a tile or a block ends the run; every TU descriptor is checked
to lie inside its planes.  What the chain and the rate leave in the workspace comes from the restatement.  What this cannot show -- those
kernels on these descriptors, the vector stores -- is what tests/test_md_full_gpu.py is for."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import md_full_util as fu  # noqa: E402
import svtav1_hip  # noqa: E402
from lr_host_util import build_host_program  # noqa: E402

SLOT = np.dtype([("row", "<u4"), ("use_row", "<u4"), ("tx_type_y", "u1"), ("tx_type_uv", "u1"), ("bad_type", "u1"), ("reserved", "u1", (5,))])
SEARCH_TU = np.dtype([("lambda_", "<u8"), ("index", "<u4", (16,)), ("tx_size", "<u4"), ("reserved", "<u4")])
TU, RATE = svtav1_hip.TU_DESC_DTYPE, svtav1_hip.COEFF_RATE_DESC_DTYPE


@pytest.fixture(scope="module")
def host_kernels(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("md_full_host")
    return build_host_program(tmp, "md_full_host"), str(tmp)


def _inside(offset, stride, w, h, shape):
    return (offset // stride + h <= shape[0]) & (offset % stride + w <= shape[1])


@pytest.mark.parametrize("name", list(fu.CASES))
def test_device_arithmetic_matches_restatement_on_the_host(host_kernels, name):
    exe, tmp = host_kernels
    s, st, sh = fu.scenario(name), fu.expected(name), fu.shared()
    n, w, h, cw, ch = s.n_slots, s.w, s.h, s.cw, s.ch
    ts_y, ts_uv = fu.tx_size_of(w, h), fu.tx_size_of(cw, ch)
    both = s.mask_inter | s.mask_intra
    types = [t for t in range(16) if both >> t & 1] if both != 1 else []
    eob, dist, bits, dc = np.zeros((3, n), np.uint16), np.zeros((3, n, 2), np.uint64), np.zeros((3, n), np.uint32), np.zeros((3, n), np.int32)
    energy = np.array([st["luma"][k]["energy"] for k in range(n)], np.uint64)
    for k in range(n):
        for p, c in enumerate([st["luma"][k]] + st["chroma"][k]):
            eob[p, k], dist[p, k], bits[p, k], dc[p, k] = c["eob"], c["dist"], c["bits"], c["dc"]
    winner = np.array([types.index(st["slots"][k]["tx_y"]) if types else 0 for k in range(n)], np.uint8)
    _, recon0 = fu.fresh_planes(s)
    for shift in (0, 3):
        head = [w, h, s.n_cand, s.n_groups, s.max_full, fu.SLOT_TILES_PER_ROW, s.mask_inter, s.mask_intra, s.reduced, shift,
                s.src[0].shape[1], s.src[1].shape[1], s.pool[0].shape[1], s.pool[1].shape[1],
                st["slot"][0].shape[1], st["slot"][0].shape[0], st["slot"][1].shape[1], st["slot"][1].shape[0],
                recon0[0].shape[1], recon0[0].shape[0], recon0[1].shape[1], recon0[1].shape[0], len(types), ts_y]
        fin, fout = os.path.join(tmp, f"{name}_{shift}_in.bin"), os.path.join(tmp, f"{name}_{shift}_out.bin")
        with open(fin, "wb") as f:
            f.write(np.array(head, np.int32).tobytes() + np.array(types + [0] * (16 - len(types)), np.uint8).tobytes()
                    + sh["iscan_offsets"][ts_y].tobytes() + sh["iscan_offsets"][ts_uv].tobytes()
                    + b"".join(a.tobytes() for a in (s.fast, s.full, s.groups, s.picks, eob, energy, dist, bits, dc, winner))
                    + b"".join(np.ascontiguousarray(p).tobytes() for p in (*st["slot"], *recon0)))
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        raw = open(fout, "rb").read()
        at = 0

        def take(dtype, count):
            nonlocal at
            a = np.frombuffer(raw, dtype, count, at)
            at += a.nbytes
            return a

        m = n * len(types)
        slots, tu, rate = take(SLOT, n), take(TU, 3 * n).reshape(3, n), take(RATE, 3 * n).reshape(3, n)
        s_tu, s_rate, s_tus, bases = take(TU, m), take(RATE, m), take(SEARCH_TU, n), take(np.uint32, 19 * 16)
        result, decision = take(fu.RESULT_DTYPE, n), take(fu.DECISION_DTYPE, s.n_groups)
        recon = [take(np.uint8, p.size).reshape(p.shape) for p in recon0]
        assert int(take(np.int32, 1)[0]) == st["refused"] and at == len(raw)

        for i, (g, want) in enumerate(zip(result, st["result"])):
            assert g == want, (name, i, g, want)
        assert np.array_equal(decision, st["decision"])
        assert all(np.array_equal(a, b) for a, b in zip(recon, st["recon"])), "the copied reconstruction differs"
        for k in range(n):
            sl = st["slots"][k]
            assert (int(slots[k]["row"]), int(slots[k]["use_row"]), int(slots[k]["tx_type_y"]), int(slots[k]["tx_type_uv"]), bool(slots[k]["bad_type"])) == \
                (sl["row"], sl["use"], sl["tx_y"], sl["tx_uv"], sl["bad"]), (name, k)

        # the descriptors: positions from the rows the slots use, every TU inside its planes, tiles and levels of no two slots overlap
        use = slots["use_row"]
        f, d = s.fast[use], s.full[use]
        k = np.arange(n)
        tile_x, tile_y = (k % fu.SLOT_TILES_PER_ROW) * s.tw, (k // fu.SLOT_TILES_PER_ROW) * s.th
        for p in range(3):
            bw_, bh_ = (w, h) if p == 0 else (cw, ch)
            r8 = (lambda v: v) if p == 0 else (lambda v: ((v >> 3) << 3) // 2)
            strides = [a[min(p, 1)].shape[1] for a in (s.src, s.pool, st["slot"])]
            want_off = [r8(f["src_y"].astype(np.int64)) * strides[0] + r8(f["src_x"].astype(np.int64)),
                        r8(f["pred_y"].astype(np.int64)) * strides[1] + r8(f["pred_x"].astype(np.int64)), r8(tile_y) * strides[2] + r8(tile_x)]
            t = tu[p]
            for field, wo, plane, stride in zip(("src_offset", "pred_offset", "recon_offset"), want_off, (s.src[p], s.pool[p], st["slot"][p]), strides):
                assert np.array_equal(t[field], wo), (name, p, field)
                assert _inside(t[field].astype(np.int64), stride, bw_, bh_, plane.shape).all(), (name, p, field)
            assert np.array_equal(t["src_stride"], np.full(n, strides[0])) and np.array_equal(t["pred_stride"], np.full(n, strides[1])) and \
                np.array_equal(t["recon_stride"], np.full(n, strides[2]))
            ncoef = min(bw_, 32) * min(bh_, 32)
            tx = slots["tx_type_y"] if p == 0 else slots["tx_type_uv"]
            assert np.array_equal(t["coeff_offset"], k * ncoef) and np.array_equal(t["tx_type"], tx)
            assert np.array_equal(t["iscan_offset"], sh["iscan_offsets"][ts_y if p == 0 else ts_uv][tx]) and np.array_equal(t["qparam_index"], d["qparam_index"][:, p])
            q = rate[p]
            assert np.array_equal(q["coeff_offset"], t["coeff_offset"]) and np.array_equal(q["iscan_offset"], t["iscan_offset"]) and np.array_equal(q["tx_type"], tx)
            assert (q["plane_type"] == min(p, 1)).all() and np.array_equal(q["txb_skip_ctx"], d["txb_skip_ctx"][:, p]) and \
                np.array_equal(q["dc_sign_ctx"], d["dc_sign_ctx"][:, p]) and np.array_equal(q["is_inter"], (f["flags"] & 16) >> 4) and \
                np.array_equal(q["intra_mode"], d["intra_mode"]) and (q["reduced_tx_set"] == s.reduced).all()
        if types:
            pos = np.arange(m)
            assert np.array_equal(s_tu["recon_offset"], pos * w * h) and (s_tu["recon_stride"] == w).all() and np.array_equal(s_tu["coeff_offset"], pos * min(w, 32) * min(h, 32))
            assert np.array_equal(s_tu["tx_type"], np.repeat(types, n)) and np.array_equal(s_tu["iscan_offset"], sh["iscan_offsets"][ts_y][np.repeat(types, n)])
            assert np.array_equal(s_tu["src_offset"], np.tile(tu[0]["src_offset"], len(types))) and np.array_equal(s_tu["pred_offset"], np.tile(tu[0]["pred_offset"], len(types)))
            assert np.array_equal(s_rate["tx_type"], s_tu["tx_type"]) and np.array_equal(s_rate["coeff_offset"], s_tu["coeff_offset"])
            want_bases = np.zeros(19 * 16, np.uint32)
            want_bases[ts_y * 16 + np.array(types)] = np.arange(len(types)) * n
            assert np.array_equal(bases, want_bases)
            inter = (f["flags"] & 16) != 0
            for t_ in range(16):
                in_mask = np.where(inter, s.mask_inter >> t_ & 1, s.mask_intra >> t_ & 1).astype(bool)
                assert np.array_equal(s_tus["index"][:, t_], np.where(in_mask, k, 0xFFFFFFFF))
            assert np.array_equal(s_tus["lambda_"], d["lambda_"]) and (s_tus["tx_size"] == ts_y).all()
