"""GPU: mode decision's full loop for the 128-wide blocks (svthip_md_full_loop128_batch_dev) through the C ABI, bit-exact against the fixture
(tests/golden/md_full128.npz) and the restatement (tests/md_full128_util.py: expected() computes a case once, asserts it equal to the fixture
and is shared by the tests).  The planes sit inside guarded garbage as in tests/test_md_full_gpu.py (_Planes: a multiple-of-4 base and stride,
and 3 bytes into the buffer at an odd stride); the slot pool, the reconstructed picture, d_result, d_tu, d_decision and d_work come back
whole, so a write outside a tile, a block, a row or the workspace shows."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import md_full128_util as wu  # noqa: E402
import md_full_util as fu  # noqa: E402
import svtav1_hip  # noqa: E402
from test_md_full_gpu import GUARD, _Call as _Call64, _check as _check64, _dev, _Planes  # noqa: E402

pytestmark = pytest.mark.gpu

BAD = "80001005"
ALL = wu.LUMA | wu.CHROMA | wu.DECIDE
SMALL_SIZES = [wh for wh in svtav1_hip.TX_SIZES_WH]   # the 19 sizes of the other entry


class _Call:
    """one scenario on the device: its arrays, planes, workspace and outputs, for one or more calls"""

    def __init__(self, torch, ctx, s, shift=0):
        self.torch, self.ctx, self.s = torch, ctx, s
        sh = fu.shared()
        slot0, recon0 = fu.fresh_planes(s)
        self.src, self.pool, self.slot, self.recon = (_Planes(torch, p, shift) for p in (s.src, s.pool, slot0, recon0))
        self.d_fast, self.d_full, self.d_group, self.d_pick = (_dev(torch, a) for a in (s.fast, s.full, s.groups, s.picks))
        self.d_qp, self.d_iscan, self.d_tables = _dev(torch, sh["qparams"]), _dev(torch, sh["tabs"].iscan_pool), _dev(torch, sh["tables"])
        self.offsets = sh["iscan_offsets"]
        self.work_bytes = svtav1_hip.md_full128_workspace_bytes(s.n_groups, s.max_full, s.w, s.h)
        assert self.work_bytes > 0
        full = lambda n: torch.full((n,), GUARD, dtype=torch.uint8, device="cuda:0")  # noqa: E731
        self.d_work, self.d_result, self.d_tu, self.d_decision = full(self.work_bytes + 64), full((s.n_slots + 1) * 144), full((s.n_slots + 1) * 32), \
            full((s.n_groups + 1) * 16)
        torch.cuda.synchronize()

    def args(self, stages):
        s = self.s
        return dict(src=self.src.arg, pred=self.pool.arg, d_fast=self.d_fast.data_ptr(), d_full=self.d_full.data_ptr(), n_cand=s.n_cand,
                    d_group=self.d_group.data_ptr(), d_pick=self.d_pick.data_ptr(), n_groups=s.n_groups, bwidth=s.w, bheight=s.h,
                    d_qparams=self.d_qp.data_ptr(), d_iscan=self.d_iscan.data_ptr(), iscan_offsets=self.offsets, d_tables=self.d_tables.data_ptr(),
                    reduced_tx_set=s.reduced, max_full=s.max_full, slot_recon=self.slot.arg, tiles_per_row=wu.SLOT_TILES_PER_ROW, recon=self.recon.arg,
                    d_work=self.d_work.data_ptr(), stages=stages, d_result=self.d_result.data_ptr(), d_tu=self.d_tu.data_ptr(),
                    d_decision=self.d_decision.data_ptr())

    def run(self, stages=ALL, stream=None):
        self.ctx.md_full_loop128_batch_dev(**self.args(stages), stream=stream)

    def finish(self):
        """(result rows, per-TU rows, decision rows, slot planes, reconstructed picture) after a synchronisation; the guards are checked"""
        self.ctx.synchronize()
        self.torch.cuda.synchronize()
        s = self.s
        raw_r, raw_t, raw_d = self.d_result.cpu().numpy(), self.d_tu.cpu().numpy(), self.d_decision.cpu().numpy()
        assert (raw_r[s.n_slots * 144:] == GUARD).all() and (raw_t[s.n_slots * 32:] == GUARD).all() and (raw_d[s.n_groups * 16:] == GUARD).all(), \
            "wrote behind the last row"
        assert (self.d_work.cpu().numpy()[self.work_bytes:] == GUARD).all(), "wrote behind the workspace"
        return (raw_r[:s.n_slots * 144].view(wu.RESULT_DTYPE), raw_t[:s.n_slots * 32].view(wu.TU_DTYPE), raw_d[:s.n_groups * 16].view(wu.DECISION_DTYPE),
                self.slot.download(), self.recon.download())


def _check(got, st, what):
    result, tu, decision, slot, recon = got
    for i, (g, w_) in enumerate(zip(result, st["result"])):
        assert g == w_, (what, "slot", i, g, w_)
    for i, (g, w_) in enumerate(zip(tu, st["tu"])):
        assert g.tobytes() == w_.tobytes(), (what, "per-TU record of slot", i, g, w_)
    assert np.array_equal(decision, st["decision"]), (what, decision, st["decision"])
    for p, (a, b) in enumerate(zip(slot, st["slot"])):
        assert np.array_equal(a, b), (what, "slot plane", p, np.argwhere(a != b)[:4])
    for p, (a, b) in enumerate(zip(recon, st["recon"])):
        assert np.array_equal(a, b), (what, "reconstructed plane", p, np.argwhere(a != b)[:4])


def _refused(ctx, n):
    if n == 0:
        assert ctx.inter_pred_refused() == 0
        return
    with pytest.raises(svtav1_hip.SvtHipError, match=rf"{BAD}: {n} PU\(s\) or unit\(s\) refused.*a pick or TxType"):
        ctx.inter_pred_refused()
    assert ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("name", list(wu.CASES))
def test_every_case_bit_exact(hip_ctx, name):
    """128x128 with 3 groups of 3 slots, 128x64 with 2 groups of 1, 64x128 with 5 groups of 12 and a group the pick refused: has_coeff masks
    with some TUs' bits, slots with every eob 0, INVALID candidates and a tx_type_uv without a network among the picks, slots past a group's
    picks; in one call, and as LUMA followed by CHROMA | DECIDE on another stream with the state in d_work and the slot tiles"""
    torch = pytest.importorskip("torch")
    s, st = wu.scenario(name), wu.expected(name)
    hip_ctx.inter_pred_refused()
    call = _Call(torch, hip_ctx, s, 0)
    call.run()
    _check(call.finish(), st, (name, "one call"))
    _refused(hip_ctx, st["refused"])
    call = _Call(torch, hip_ctx, s, 3)
    call.run(wu.LUMA)
    stream = torch.cuda.Stream()
    call.run(wu.CHROMA | wu.DECIDE, stream=stream.cuda_stream)
    stream.synchronize()
    _check(call.finish(), st, (name, "two calls"))
    _refused(hip_ctx, st["refused"])


def test_one_context_across_sizes_and_entries():
    """128x128, then the other entry at 64x64, then 64x128 and 128x64 on one context: each equals its own expectation"""
    torch = pytest.importorskip("torch")
    ctx = svtav1_hip.Context(0)
    try:
        for name in ("128x128", "64x64", "64x128", "128x64"):
            if name == "64x64":
                call = _Call64(torch, ctx, fu.scenario(name), 0)
                call.run()
                _check64(call.finish(), fu.expected(name), "64x64 between two calls of the 128-wide entry")
                assert ctx.inter_pred_refused() == fu.expected(name)["refused"] == 0
                continue
            st = wu.expected(name)
            call = _Call(torch, ctx, wu.scenario(name), 1)
            call.run()
            _check(call.finish(), st, name)
            _refused(ctx, st["refused"])
    finally:
        ctx.close()


def test_refusals():
    torch = pytest.importorskip("torch")
    ctx = svtav1_hip.Context(0)
    try:
        s = wu.scenario("128x64")
        call = _Call(torch, ctx, s, 0)
        ok = call.args(ALL)
        full = ctx.md_full_loop128_batch_dev

        def refused(words, **change):
            with pytest.raises(svtav1_hip.SvtHipError, match=f"{BAD}.*{words}"):
                full(**{**ok, **change})

        assert len(SMALL_SIZES) == 19
        for bw, bh in SMALL_SIZES + [(0, 0), (256, 128)]:
            refused("not one of the block sizes 128x128, 128x64 and 64x128", bwidth=bw, bheight=bh)
            assert svtav1_hip.md_full128_workspace_bytes(2, 1, bw, bh) == 0
        refused("128x128, 128x64 and 64x128", bwidth=64, bheight=64, n_groups=0)   # the size is checked before the count
        for bw, bh in ((128, 128), (128, 64), (64, 128)):
            assert svtav1_hip.md_full128_workspace_bytes(2, 1, bw, bh) > 0
        # the remaining refusals are those of the other entry
        for stages in (0, 8, 15):
            refused("stages must be a mask", stages=stages)
        for max_full in (0, 13):
            refused("max_full must be 1..12", max_full=max_full)
            assert svtav1_hip.md_full128_workspace_bytes(2, max_full, 128, 64) == 0
        refused("tiles_per_row must not be 0", tiles_per_row=0)
        for k in ("src", "pred", "slot_recon", "recon", "d_fast", "d_full", "d_group", "d_pick", "d_qparams", "d_iscan", "iscan_offsets", "d_tables", "d_work",
                  "d_result", "d_tu", "d_decision"):
            refused("null pointer", **{k: None})
        for which in ("src", "pred", "slot_recon", "recon"):
            for field, value, words in (("cr", None, "null plane pointer"), ("y_stride", 65536, "plane strides must be at most 65535")):
                p = svtav1_hip.InterPlanes()
                for f in ("y", "cb", "cr", "y_stride", "c_stride"):
                    setattr(p, f, getattr(ok[which], f))
                setattr(p, field, value)
                refused(words, **{which: p})
        refused("n_cand must not be 0", n_cand=0)
        refused("descriptor array must be 16-byte aligned", d_fast=ok["d_fast"] + 8)
        for k in ("d_full", "d_pick", "d_work", "d_result", "d_tu", "d_decision"):
            refused("must be 16-byte aligned", **{k: ok[k] + 8})
        refused("group array must be 8-byte aligned", d_group=ok["d_group"] + 4)
        refused("iscan pool must be 8-byte aligned", d_iscan=ok["d_iscan"] + 2)
        refused("too many slots in one call", tiles_per_row=512)
        full(**{**{k: None for k in ok}, "n_groups": 0, "bwidth": 128, "bheight": 128, "max_full": 4, "tiles_per_row": 1, "stages": ALL, "n_cand": 0,
                "reduced_tx_set": 0})   # n_groups == 0 returns OK
        ctx.synchronize()
        assert ctx.inter_pred_refused() == 0
        # nothing above launched: the outputs are untouched, and the context still computes
        call.run()
        _check(call.finish(), wu.expected("128x64"), "after the refusals")
        _refused(ctx, wu.expected("128x64")["refused"])
    finally:
        ctx.close()
