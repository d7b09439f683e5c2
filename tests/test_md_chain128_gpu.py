"""GPU: the hand-over at 128x128 on device-made data, one stream: av1_inter_pred_batch_dev (two blocks of a 256x128 picture, three
candidates each, into the pool) -> md_fast_cost_batch_dev -> md_fast_pick_batch_dev -> md_full_loop128_batch_dev, against the same stages of
the restatements (tests/md_full128_util.py: run_chain).  Nothing is read back between the calls: the full loop reads the pool and the picks
the calls in front of it left in device memory."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import inter_pred_util as ipu  # noqa: E402
import md_fast_util as mu  # noqa: E402
import md_full128_util as wu  # noqa: E402
import md_full_util as fu  # noqa: E402
import svtav1_hip  # noqa: E402
from test_md_full_gpu import GUARD, _dev, _Planes  # noqa: E402

pytestmark = pytest.mark.gpu


def test_chain_at_128x128(hip_ctx, oracle):
    torch = pytest.importorskip("torch")
    s = wu.chain_scenario()
    pool0 = [p.copy() for p in s.pool]
    want = wu.run_chain(oracle, s)
    st = want["state"]
    assert [sl["row"] != wu.NONE for sl in st["slots"]] == [True, True, False, True, True, True] and st["refused"] == 0
    assert any(0 < int(r["y_has_coeff"]) for r in st["result"]) and all(int(d["winner_row"]) != wu.NONE for d in st["decision"])
    sh = fu.shared()
    hip_ctx.inter_pred_refused()
    slot0, recon0 = fu.fresh_planes(s)
    src, pool, slot, recon = (_Planes(torch, p, shift) for p, shift in ((s.src, 0), (pool0, 1), (slot0, 2), (recon0, 3)))
    refs = [ipu.to_device(p) for p in (s.ref0, s.ref1)]
    ref_args = [ipu.planes_of(d, p) for d, p in zip(refs, (s.ref0, s.ref1))]
    d_pu, d_fast, d_full, d_group = (_dev(torch, a) for a in (s.pu, s.fast, s.full, s.groups))
    d_qp, d_iscan, d_tables = _dev(torch, sh["qparams"]), _dev(torch, sh["tabs"].iscan_pool), _dev(torch, sh["tables"])
    full = lambda n: torch.full((n,), GUARD, dtype=torch.uint8, device="cuda:0")  # noqa: E731
    work_bytes = svtav1_hip.md_full128_workspace_bytes(s.n_groups, s.max_full, s.w, s.h)
    d_fast_result, d_pick, d_work = full(7 * 16), full(3 * 32), full(work_bytes + 64)
    d_result, d_tu, d_decision = full(7 * 144), full(7 * 32), full(3 * 16)
    torch.cuda.synchronize()
    hip_ctx.av1_inter_pred_batch_dev(ref_args[0], ref_args[1], pool.arg, d_pu.data_ptr(), 6, s.w, s.h)
    hip_ctx.md_fast_cost_batch_dev(src.arg, pool.arg, d_fast.data_ptr(), 6, s.w, s.h, d_fast_result.data_ptr())
    hip_ctx.md_fast_pick_batch_dev(d_fast_result.data_ptr(), d_fast.data_ptr(), 6, d_group.data_ptr(), 2, d_pick.data_ptr())
    hip_ctx.md_full_loop128_batch_dev(src.arg, pool.arg, d_fast.data_ptr(), d_full.data_ptr(), 6, d_group.data_ptr(), d_pick.data_ptr(), 2, s.w, s.h,
                                      d_qp.data_ptr(), d_iscan.data_ptr(), sh["iscan_offsets"], d_tables.data_ptr(), 0, s.max_full, slot.arg,
                                      wu.SLOT_TILES_PER_ROW, recon.arg, d_work.data_ptr(), wu.LUMA | wu.CHROMA | wu.DECIDE, d_result.data_ptr(),
                                      d_tu.data_ptr(), d_decision.data_ptr())
    hip_ctx.synchronize()
    torch.cuda.synchronize()
    rows = lambda t, n, dt: (t.cpu().numpy()[:n * dt.itemsize].view(dt), t.cpu().numpy()[n * dt.itemsize:])  # noqa: E731
    for what, t, n, dt, w_ in (("fast cost", d_fast_result, 6, mu.RESULT_DTYPE, want["fast"]), ("pick", d_pick, 2, mu.PICK_DTYPE, want["picks"]),
                               ("full loop result", d_result, 6, wu.RESULT_DTYPE, st["result"]), ("full loop per-TU record", d_tu, 6, wu.TU_DTYPE, st["tu"]),
                               ("full loop decision", d_decision, 2, wu.DECISION_DTYPE, st["decision"])):
        got, guard = rows(t, n, dt)
        assert (guard == GUARD).all(), f"wrote behind the last row of the {what}"
        assert got.tobytes() == np.ascontiguousarray(w_).tobytes(), (what, got, w_)
    assert (d_work.cpu().numpy()[work_bytes:] == GUARD).all(), "wrote behind the workspace"
    for what, planes, w_ in (("inter prediction", pool, want["pool"]), ("slot tiles", slot, st["slot"]), ("reconstructed picture", recon, st["recon"]),
                             ("source", src, s.src)):
        for p, (a, b) in enumerate(zip(planes.download(), w_)):
            assert np.array_equal(a, b), (what, "plane", p, np.argwhere(a != b)[:4])
    assert hip_ctx.inter_pred_refused() == 0
