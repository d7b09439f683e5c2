"""GPU: mode decision's full loop (svthip_md_full_loop_batch_dev) through the C ABI, bit-exact against the fixture (tests/golden/md_full.npz) and
the restatement (tests/md_full_util.py: expected() computes a case once, asserts it equal to the fixture and is shared by the tests).  Every
plane -- source, prediction pool, slot pool, reconstructed picture -- sits inside a larger buffer of garbage, once with a stride and a base
that are multiples of 4 and once each 1, 2 and 3 bytes into its buffer at an odd stride; the buffers of the slot pool and of the
reconstructed picture, d_result, d_decision and d_work come back whole, so a write outside a tile, a block, a row or the workspace shows."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import md_full_util as fu  # noqa: E402
import svtav1_hip  # noqa: E402

pytestmark = pytest.mark.gpu

BAD = "80001005"
ALL = fu.LUMA | fu.CHROMA | fu.DECIDE
GUARD = 0x77


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


class _Planes:
    """Y, Cb, Cr inside garbage on the device; Cb and Cr share a stride"""

    def __init__(self, torch, planes, shift):
        self.torch, self.shapes, self.shift, self.host, self.dev, self.strides = torch, [p.shape for p in planes], shift, [], [], []
        for k, p in enumerate(planes):
            h, w = p.shape
            wide = planes[1].shape[1] if k else w
            stride = (wide + 11) // 4 * 4 if shift == 0 else (wide + 8) | 1
            buf = np.full((h + 2) * stride + 8, 0x3C, np.uint8)
            buf[1::3] = 0xC3
            buf[stride + shift:stride + shift + h * stride].reshape(h, stride)[:, :w] = p
            self.host.append(buf)
            self.dev.append(_dev(torch, buf))
            self.strides.append(stride)
        self.arg = svtav1_hip.InterPlanes()
        self.arg.y, self.arg.cb, self.arg.cr = (t.data_ptr() + s + shift for t, s in zip(self.dev, self.strides))
        self.arg.y_stride, self.arg.c_stride = self.strides[0], self.strides[1]

    def upload(self, planes):
        """new contents for the planes, in place"""
        for buf, t, stride, p in zip(self.host, self.dev, self.strides, planes):
            h, w = p.shape
            buf[stride + self.shift:stride + self.shift + h * stride].reshape(h, stride)[:, :w] = p
            t.copy_(self.torch.from_numpy(buf))

    def download(self):
        """the planes; asserts that nothing around them changed"""
        out = []
        for buf, t, stride, (h, w) in zip(self.host, self.dev, self.strides, self.shapes):
            got = t.cpu().numpy()
            rows = got[stride + self.shift:stride + self.shift + h * stride].reshape(h, stride)
            out.append(rows[:, :w].copy())
            want = buf.copy()
            want[stride + self.shift:stride + self.shift + h * stride].reshape(h, stride)[:, :w] = out[-1]
            assert np.array_equal(got, want), "wrote outside the plane"
        return out


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
        self.work_bytes = svtav1_hip.md_full_workspace_bytes(s.n_groups, s.max_full, s.w, s.h, s.mask_inter, s.mask_intra)
        assert self.work_bytes > 0
        self.d_work = torch.full((self.work_bytes + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
        self.d_result = torch.full(((s.n_slots + 1) * 144,), GUARD, dtype=torch.uint8, device="cuda:0")
        self.d_decision = torch.full(((s.n_groups + 1) * 16,), GUARD, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

    def args(self, stages):
        s = self.s
        return dict(src=self.src.arg, pred=self.pool.arg, d_fast=self.d_fast.data_ptr(), d_full=self.d_full.data_ptr(), n_cand=s.n_cand,
                    d_group=self.d_group.data_ptr(), d_pick=self.d_pick.data_ptr(), n_groups=s.n_groups, bwidth=s.w, bheight=s.h,
                    d_qparams=self.d_qp.data_ptr(), d_iscan=self.d_iscan.data_ptr(), iscan_offsets=self.offsets, d_tables=self.d_tables.data_ptr(),
                    reduced_tx_set=s.reduced, type_mask_inter=s.mask_inter, type_mask_intra=s.mask_intra, max_full=s.max_full, slot_recon=self.slot.arg,
                    tiles_per_row=fu.SLOT_TILES_PER_ROW, recon=self.recon.arg, d_work=self.d_work.data_ptr(), stages=stages,
                    d_result=self.d_result.data_ptr(), d_decision=self.d_decision.data_ptr())

    def run(self, stages=ALL, stream=None):
        self.ctx.md_full_loop_batch_dev(**self.args(stages), stream=stream)

    def finish(self):
        """(result rows, decision rows, slot planes, reconstructed picture) after a synchronisation; the guards are checked"""
        self.ctx.synchronize()
        self.torch.cuda.synchronize()
        s = self.s
        raw_r, raw_d = self.d_result.cpu().numpy(), self.d_decision.cpu().numpy()
        assert (raw_r[s.n_slots * 144:] == GUARD).all() and (raw_d[s.n_groups * 16:] == GUARD).all(), "wrote behind the last row"
        assert (self.d_work.cpu().numpy()[self.work_bytes:] == GUARD).all(), "wrote behind the workspace"
        return raw_r[:s.n_slots * 144].view(fu.RESULT_DTYPE), raw_d[:s.n_groups * 16].view(fu.DECISION_DTYPE), self.slot.download(), self.recon.download()


def _check(got, st, what):
    result, decision, slot, recon = got
    for i, (g, w_) in enumerate(zip(result, st["result"])):
        assert g == w_, (what, "slot", i, g, w_)
    assert np.array_equal(decision, st["decision"]), (what, decision, st["decision"])
    for p, (a, b) in enumerate(zip(slot, st["slot"])):
        assert np.array_equal(a, b), (what, "slot plane", p, np.argwhere(a != b)[:4])
    for p, (a, b) in enumerate(zip(recon, st["recon"])):
        assert np.array_equal(a, b), (what, "reconstructed plane", p, np.argwhere(a != b)[:4])


def _refused(ctx, n):
    if n == 0:
        assert ctx.inter_pred_refused() == 0
        return
    with pytest.raises(svtav1_hip.SvtHipError, match=rf"{BAD}: {n} PU\(s\) or unit\(s\) refused.*svthip_md_full_loop_batch_dev"):
        ctx.inter_pred_refused()
    assert ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("name", list(fu.CASES))
def test_every_case_bit_exact(hip_ctx, name):
    """the seven sizes (4x4 with mixed has_uv and the 8-pitch tiles, 64x64 with three_quad_energy and a left shift), n_groups 1, 5 and 23 with
    max_full 12 (276 slots) and max_full 1, no search, the M0 and the M1 masks, INTER and INTRA candidates, INVALID candidates among the picks,
    groups with fewer active slots than max_full, a group the pick refused"""
    torch = pytest.importorskip("torch")
    s, st = fu.scenario(name), fu.expected(name)
    hip_ctx.inter_pred_refused()
    for shift in ((0, 1, 2, 3) if s.n_groups == 5 and s.max_full == 4 else (0, 3)):
        call = _Call(torch, hip_ctx, s, shift)
        call.run()
        _check(call.finish(), st, (name, shift))
        _refused(hip_ctx, st["refused"])


@pytest.mark.parametrize("name", ["4x4", "8x8", "64x64", "8x8_g23_m12", "16x8_g5_m12_none"])
def test_two_calls_equal_one(hip_ctx, name):
    """stages = LUMA, then CHROMA | DECIDE on another stream: the state in between is in d_work and slot_recon"""
    torch = pytest.importorskip("torch")
    s, st = fu.scenario(name), fu.expected(name)
    hip_ctx.inter_pred_refused()
    call = _Call(torch, hip_ctx, s, 0)
    call.run(fu.LUMA)
    stream = torch.cuda.Stream()
    call.run(fu.CHROMA | fu.DECIDE, stream=stream.cuda_stream)
    stream.synchronize()
    _check(call.finish(), st, name)
    _refused(hip_ctx, st["refused"])
    # and the three stages one by one
    call = _Call(torch, hip_ctx, s, 3)
    for stage in (fu.LUMA, fu.CHROMA, fu.DECIDE):
        call.run(stage)
    _check(call.finish(), st, name)
    _refused(hip_ctx, st["refused"])


@pytest.mark.parametrize("name", ["8x8", "32x32"])
def test_chroma_rewritten_between_the_calls(hip_ctx, oracle, name):
    """the UV_CFL_PRED service: after LUMA the host overwrites the chroma prediction tile of one candidate and its chroma_rate"""
    torch = pytest.importorskip("torch")
    s = copy.deepcopy(fu.scenario(name))
    st = fu.full_loop(oracle, s, fu.LUMA)
    k = next(k for k in range(s.n_slots) if st["slots"][k]["row"] != fu.NONE and s.fast[st["slots"][k]["row"]]["has_uv"]
             and not (s.fast[st["slots"][k]["row"]]["flags"] & 4))
    row = st["slots"][k]["row"]
    hip_ctx.inter_pred_refused()
    call = _Call(torch, hip_ctx, s, 1)
    call.run(fu.LUMA)
    hip_ctx.synchronize()
    px, py = fu.round_uv(int(s.fast[row]["pred_x"])), fu.round_uv(int(s.fast[row]["pred_y"]))
    rng = np.random.default_rng(5)
    for p in (1, 2):
        s.pool[p][py:py + s.ch, px:px + s.cw] = rng.integers(0, 256, (s.ch, s.cw))
    s.full[row]["chroma_rate"] += 4321
    call.pool.upload(s.pool)
    call.d_full.copy_(_dev(torch, s.full))
    torch.cuda.synchronize()
    call.run(fu.CHROMA | fu.DECIDE)
    st = fu.full_loop(oracle, s, fu.CHROMA | fu.DECIDE, st)
    assert st["result"][k].tobytes() != fu.expected(name)["result"][k].tobytes()
    _check(call.finish(), st, name)
    _refused(hip_ctx, st["refused"])


def test_tx_type_without_a_network_is_counted(hip_ctx, oracle):
    """64x64: Cb / Cr are 32x32, which has no ADST; the slot runs as DCT_DCT, its cost is ~0 and the context counts it"""
    torch = pytest.importorskip("torch")
    s = copy.deepcopy(fu.scenario("64x64"))
    first = fu.expected("64x64")
    rows = sorted({sl["row"] for sl in first["slots"] if sl["row"] != fu.NONE})[:2]
    s.full["tx_type_uv"][rows[0]], s.full["tx_type_y"][rows[1]] = 1, 9
    st = fu.full_loop(oracle, s)
    bad = sum(sl["bad"] and sl["row"] != fu.NONE for sl in st["slots"])
    assert bad >= 2 and st["refused"] == first["refused"] + bad
    hip_ctx.inter_pred_refused()
    call = _Call(torch, hip_ctx, s, 0)
    call.run()
    got = call.finish()
    _check(got, st, "64x64 with bad types")
    assert all(int(r["full_cost"]) == fu.U64 for r, sl in zip(got[0], st["slots"]) if sl["bad"])
    _refused(hip_ctx, st["refused"])


def test_context_reuse_and_refusals():
    torch = pytest.importorskip("torch")
    ctx = svtav1_hip.Context(0)
    try:
        s = fu.scenario("16x8_g5_m1")
        call = _Call(torch, ctx, s, 0)
        ok = call.args(ALL)
        full = ctx.md_full_loop_batch_dev

        def refused(words, **change):
            with pytest.raises(svtav1_hip.SvtHipError, match=f"{BAD}.*{words}"):
                full(**{**ok, **change})

        for bw, bh in ((128, 128), (64, 128), (8, 64), (12, 8), (0, 0)):
            refused("not one of the 19 AV1 block sizes", bwidth=bw, bheight=bh)
            assert svtav1_hip.md_full_workspace_bytes(5, 4, bw, bh, 1, 1) == 0
        refused("not one of the 19 AV1 block sizes", bwidth=128, bheight=128, n_groups=0)   # the size is checked before the count
        for stages in (0, 8, 15):
            refused("stages must be a mask", stages=stages)
        for max_full in (0, 13):
            refused("max_full must be 1..12", max_full=max_full)
            assert svtav1_hip.md_full_workspace_bytes(5, max_full, 16, 8, 1, 1) == 0
        refused("tiles_per_row must not be 0", tiles_per_row=0)
        for masks in ((0, 1), (1, 0), (0x10001, 1), (1, 0x20000)):
            refused("a type mask is 0, has bits above 15", type_mask_inter=masks[0], type_mask_intra=masks[1])
        refused("names a TxType 64 x 64 has no network for", bwidth=64, bheight=64, type_mask_inter=3)
        assert svtav1_hip.md_full_workspace_bytes(5, 4, 64, 64, 3, 1) == 0 and svtav1_hip.md_full_workspace_bytes(5, 4, 64, 64, 1, 1) > 0
        for k in ("src", "pred", "slot_recon", "recon", "d_fast", "d_full", "d_group", "d_pick", "d_qparams", "d_iscan", "iscan_offsets", "d_tables", "d_work",
                  "d_result", "d_decision"):
            refused("null pointer", **{k: None})
        for which in ("src", "pred", "slot_recon", "recon"):
            for plane in ("y", "cb", "cr"):
                p = svtav1_hip.InterPlanes()
                for f in ("y", "cb", "cr", "y_stride", "c_stride"):
                    setattr(p, f, getattr(ok[which], f))
                setattr(p, plane, None)
                refused("null plane pointer", **{which: p})
            for stride in ("y_stride", "c_stride"):
                p = svtav1_hip.InterPlanes()
                for f in ("y", "cb", "cr", "y_stride", "c_stride"):
                    setattr(p, f, getattr(ok[which], f))
                setattr(p, stride, 65536)
                refused("plane strides must be at most 65535", **{which: p})
        refused("n_cand must not be 0", n_cand=0)
        refused("descriptor array must be 16-byte aligned", d_fast=ok["d_fast"] + 8)
        for k in ("d_full", "d_pick", "d_work", "d_result", "d_decision"):
            refused("must be 16-byte aligned", **{k: ok[k] + 8})
        refused("group array must be 8-byte aligned", d_group=ok["d_group"] + 4)
        refused("iscan pool must be 8-byte aligned", d_iscan=ok["d_iscan"] + 2)
        refused("too many slots in one call", tiles_per_row=4096)
        full(**{**{k: None for k in ok}, "n_groups": 0, "bwidth": 16, "bheight": 8, "type_mask_inter": 1, "type_mask_intra": 1, "max_full": 4,
                "tiles_per_row": 1, "stages": ALL, "n_cand": 0, "reduced_tx_set": 0})   # n_groups == 0 returns OK
        ctx.synchronize()
        assert ctx.inter_pred_refused() == 0
        # nothing above launched: the outputs are untouched, and the context still computes; then a second size on the same context
        call.run()
        _check(call.finish(), fu.expected("16x8_g5_m1"), "after the refusals")
        s2 = fu.scenario("4x16")
        call2 = _Call(torch, ctx, s2, 2)
        call2.run()
        _check(call2.finish(), fu.expected("4x16"), "second size")
        assert ctx.inter_pred_refused() == 0
    finally:
        ctx.close()
