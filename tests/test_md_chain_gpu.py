"""GPU: the mode-decision entries as the chain they were built to be, against tests/golden/md_chain.npz and the restated chain
(tests/md_chain_util.py), one luma size per chain, every call on one stream:

  md_interp_filter_search_batch_dev (write_back = 1, on the searched prefix of the PU descriptors) -> av1_inter_pred_batch_dev (every PU,
  into the pool) -> av1_intra_pred_batch_dev x 3 (Y, Cb, Cr, edges from the neighbour picture, into the same pool planes) ->
  md_fast_cost_batch_dev -> md_fast_pick_batch_dev -> md_full_loop_batch_dev(LUMA) -> the CfL service (av1_cfl_alpha_candidates_batch_dev
  on slot_recon.y and the pool's DC tiles -> encode_tu_batch_dev and coeff_rate_batch_dev on the 66 tiles a block ->
  cfl_alpha_decision_batch_dev -> av1_cfl_pred_batch_dev in place on the pool's Cb and Cr, chroma_rate of those rows uploaded) ->
  md_full_loop_batch_dev(CHROMA | DECIDE)

The header leaves two look-ups to the host -- which row a slot holds (from the picks) and the rate of the chosen alpha -- so the chain has
exactly two host reads between its first call and its last: d_pick after the LUMA stage and d_out of the alpha decision inside the CfL
service, each a copy enqueued on the chain's own stream and waited for on that stream alone; a size without CfL has none.  What the host
makes of them goes back up on the same stream.  Nothing else is downloaded before the end and no plane leaves the device: every other
array is read only in check(), after one wait, in chain order, and the first stage that differs is named.

Every plane set -- source, references, neighbour picture, pool, slot pool, reconstructed picture -- sits inside guarded garbage with a
stride of its own (tests/test_md_full_gpu.py: _Planes), on the context's stream 1, 2 or 3 bytes into its buffer at an odd stride; the
columns that set the strides apart are guard too, checked from the true width of every plane on.  Every array has a guard row and d_work
its 64 guard bytes.  What the CfL service leaves between its entries (candidate tiles, levels, eobs, distortions, rates) is compared with
the restated chain in front of the decisions, so a difference inside the service names the entry.  The busy work of the caller-stream tests is that of
tests/test_post_filter_chain_gpu.py: it can only make a misplaced launch visible, it cannot fail a correct run."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import cfl_util as cu  # noqa: E402
import md_chain_util as mc  # noqa: E402
import md_fast_util as mu  # noqa: E402
import md_full_util as fu  # noqa: E402
import md_ifs_util as su  # noqa: E402
import rate_util  # noqa: E402
import svtav1_hip  # noqa: E402
from lr_gpu_util import _ready  # noqa: E402
from test_md_full_gpu import GUARD, _dev, _Planes  # noqa: E402
from test_post_filter_chain_gpu import GATE_STEPS, _gate  # noqa: E402

pytestmark = pytest.mark.gpu

BAD = "80001005"
STAGES = ("filter search", "inter prediction", "intra prediction", "fast cost", "pick", "full loop LUMA", "CfL service", "full loop CHROMA | DECIDE")
# columns added to the planes of a set (luma twice as many), so that no two sets of a chain share a stride; _Planes takes them for
# samples of the plane, so check() asserts that they still hold PAD: the guard starts at the true width of every plane
EXTRA = {"src": 0, "ref0": 0, "ref1": 4, "nb": 4, "recon": 8, "pool": 12, "slot": 40}
PAD = 0x99
# what the CfL service leaves between its entries, in the order they are written: (name in the restated chain, what it is)
CFL_INSIDE = (("cfl_cand", "the alpha candidates' tiles"), ("cfl_recon", "the fused chain's reconstructions"), ("cfl_q", "the fused chain's levels"),
              ("cfl_eob", "the fused chain's eobs"), ("cfl_dist", "the fused chain's distortions"), ("cfl_bits", "the coefficient rates"))


def _widen(planes, extra):
    return [np.pad(p, ((0, 0), (0, extra * (2 if k == 0 else 1))), constant_values=PAD) for k, p in enumerate(planes)]


class _PlanesInOne(_Planes):
    """_Planes with the three buffers in one allocation, one after the other: a TU descriptor reaches Cb and Cr from one pointer"""

    def __init__(self, torch, planes, shift):
        super().__init__(torch, planes, shift)
        self.whole = torch.cat(self.dev)
        self.dev = list(self.whole.split([len(b) for b in self.host]))
        self.arg.y, self.arg.cb, self.arg.cr = (t.data_ptr() + s + shift for t, s in zip(self.dev, self.strides))

    def sample0(self, k):
        """offset of sample (0, 0) of plane k from the allocation's first byte"""
        return sum(len(b) for b in self.host[:k]) + self.strides[k] + self.shift


class _Array:
    """rows of a structured array on the device with one guard row behind them"""

    def __init__(self, torch, dtype, n, host=None):
        self.dtype, self.n = np.dtype(dtype), n
        raw = np.full((n + 1) * self.dtype.itemsize, GUARD, np.uint8)
        if host is not None:
            raw[:n * self.dtype.itemsize] = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        self.t = _dev(torch, raw)
        self.ptr = self.t.data_ptr()

    def _rows(self, raw):
        return raw[:self.n * self.dtype.itemsize].view(self.dtype.base).reshape((self.n,) + self.dtype.shape)

    def upload(self, torch, host, stream):
        """rows 0 .. len(host) from the host, enqueued on `stream`"""
        raw = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).reshape(-1).copy())
        with torch.cuda.stream(stream):
            self.t[:len(raw)].copy_(raw)

    def read(self, torch, stream):
        """the rows, by a copy enqueued on `stream` and waited for on that stream alone"""
        with torch.cuda.stream(stream):
            raw = self.t.cpu().numpy()
        return self._rows(raw)

    def get(self, what, used=None):
        """after the wait: the rows; asserts the guard row, and that rows from `used` on were not written"""
        raw = self.t.cpu().numpy()
        assert (raw[(self.n if used is None else used) * self.dtype.itemsize:] == GUARD).all(), f"wrote behind the last row of {what}"
        return self._rows(raw)


class DevChain:
    """one size on the device with every buffer and array of the chain, and the chain as a list of calls"""

    def __init__(self, torch, oracle, name, shift=0):
        self.torch, self.oracle, self.name, self.shift = torch, oracle, name, shift
        s = self.s = mc.make_scenario(name)
        self.want = mc.expected(name)
        for k, v in mc.input_digests(s).items():
            assert np.array_equal(v, self.want["sha256_" + k]), f"size {name}: the regenerated {k} is not the fixture's input"
        sh = self.sh = fu.shared()
        P = lambda planes, k, cls=_Planes: cls(torch, _widen(planes, EXTRA[k]), shift)  # noqa: E731
        self.host = {"src": s.src, "ref0": [s.ref0.y, s.ref0.cb, s.ref0.cr], "ref1": [s.ref1.y, s.ref1.cb, s.ref1.cr], "nb": s.nb, "pool": [p.copy() for p in s.pool]}
        self.host["slot"], self.host["recon"] = fu.fresh_planes(s)
        self.planes = {k: P(v, k, _PlanesInOne if k == "src" else _Planes) for k, v in self.host.items()}
        assert all(len({p.strides[k] for p in self.planes.values()}) == len(self.planes) for k in (0, 1)), "two plane sets share a stride"
        self.refs = [self._inside(self.planes[k], s.ref0.border) for k in ("ref0", "ref1")]
        A = lambda dtype, n, host=None: _Array(torch, dtype, n, host)  # noqa: E731
        self.pu0, self.fast0, self.full0 = s.pu.copy(), s.fast.copy(), s.full.copy()
        self.d_pu, self.d_ifs_desc, self.d_ifs = A(s.pu.dtype, len(s.pu), s.pu), A(su.IFS_DESC_DTYPE, s.n_search, s.ifs_desc), A(su.IFS_RESULT_DTYPE, s.n_search)
        self.d_intra = []
        for p in range(3):
            nb, pool = self.planes["nb"], self.planes["pool"]
            d, ts = mc.intra_descs(s, p, nb.strides[p], nb.strides[p] + shift, pool.strides[p], pool.strides[p] + shift)
            self.d_intra.append((A(d.dtype, len(d), d), len(d), ts))
        self.d_fast, self.d_full, self.d_group = A(s.fast.dtype, s.n_cand, s.fast), A(s.full.dtype, s.n_cand, s.full), A(s.groups.dtype, s.n_groups, s.groups)
        self.d_fast_result, self.d_pick = A(mu.RESULT_DTYPE, s.n_cand), A(mu.PICK_DTYPE, s.n_groups)
        self.d_qp, self.d_iscan, self.d_tables = _dev(torch, sh["qparams"]), _dev(torch, sh["tabs"].iscan_pool), _dev(torch, sh["tables"])
        self.work_bytes = svtav1_hip.md_full_workspace_bytes(s.n_groups, s.max_full, s.w, s.h, s.mask_inter, s.mask_intra)
        assert self.work_bytes > 0
        self.d_work = torch.full((self.work_bytes + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
        self.d_result, self.d_decision = A(fu.RESULT_DTYPE, s.n_slots), A(fu.DECISION_DTYPE, s.n_groups)
        # the CfL service: room for every slot
        n, npx = (s.n_slots if s.cfl else 0), s.cw * s.ch
        self.d_cfl_desc, self.d_cfl_chosen, self.d_job, self.d_cfl = A(cu.DESC, n), A(cu.DESC, n), A(cu.JOB, n), A(cu.DECISION, n)
        self.d_tu, self.d_rd = A(svtav1_hip.TU_DESC_DTYPE, n * 66), A(svtav1_hip.COEFF_RATE_DESC_DTYPE, n * 66)
        self.d_cand, self.d_cand_recon = A(np.dtype(("u1", (npx,))), n * 66), A(np.dtype(("u1", (npx,))), n * 66)
        self.d_q, self.d_eob = A(np.dtype(("<i4", (npx,))), n * 66), A(np.uint16, n * 66)
        self.d_dist, self.d_bits = A(np.dtype(("<u8", (2,))), n * 66), A(np.uint32, n * 66)
        self.d_alpha_bits = _dev(torch, np.asarray(s.alpha_bits, np.int32))
        self.cfl_slots, self.n_cfl = [], 0
        _ready(torch)

    @staticmethod
    def _inside(p, border):
        """InterPlanes at picture sample (0, 0) of a padded picture"""
        a = svtav1_hip.InterPlanes()
        a.y, a.cb, a.cr = p.arg.y + border * p.strides[0] + border, p.arg.cb + (border // 2) * (p.strides[1] + 1), p.arg.cr + (border // 2) * (p.strides[1] + 1)
        a.y_stride, a.c_stride = p.strides[0], p.strides[1]
        return a

    def _full_loop(self, ctx, stages, stream):
        s, pl = self.s, self.planes
        ctx.md_full_loop_batch_dev(src=pl["src"].arg, pred=pl["pool"].arg, d_fast=self.d_fast.ptr, d_full=self.d_full.ptr, n_cand=s.n_cand, d_group=self.d_group.ptr,
                                   d_pick=self.d_pick.ptr, n_groups=s.n_groups, bwidth=s.w, bheight=s.h, d_qparams=self.d_qp.data_ptr(),
                                   d_iscan=self.d_iscan.data_ptr(), iscan_offsets=self.sh["iscan_offsets"], d_tables=self.d_tables.data_ptr(), reduced_tx_set=s.reduced,
                                   type_mask_inter=s.mask_inter, type_mask_intra=s.mask_intra, max_full=s.max_full, slot_recon=pl["slot"].arg,
                                   tiles_per_row=fu.SLOT_TILES_PER_ROW, recon=pl["recon"].arg, d_work=self.d_work.data_ptr(), stages=stages,
                                   d_result=self.d_result.ptr, d_decision=self.d_decision.ptr, stream=stream)

    def _cfl_service(self, ctx, stream):
        """step 7, with the chain's two host reads"""
        s, pl, torch = self.s, self.planes, self.torch
        if not s.cfl:
            return
        S = torch.cuda.ExternalStream(stream if stream is not None else ctx.stream)
        picks = self.d_pick.read(torch, S)                                       # host read 1: which row a slot holds
        rows = mc.slot_rows(s, picks)
        slots = self.cfl_slots = mc.cfl_slots(s, rows)
        n = self.n_cfl = len(slots)
        if n == 0:
            return
        slot, pool, src = pl["slot"], pl["pool"], pl["src"]
        desc = mc.cfl_descs(s, slots, rows, slot.strides[0], slot.strides[0] + self.shift, pool.strides[1], pool.strides[1] + self.shift)
        tu, rd, jobs = mc.cfl_tu_descs(s, slots, rows, src.strides[1], src.sample0(1), src.sample0(2))
        for a, host in ((self.d_cfl_desc, desc), (self.d_tu, tu), (self.d_rd, rd), (self.d_job, jobs)):
            a.upload(torch, host, S)
        luma, cb, cr = slot.dev[0].data_ptr(), pool.dev[1].data_ptr(), pool.dev[2].data_ptr()
        ctx.av1_cfl_alpha_candidates_batch_dev(luma, cb, cr, self.d_cfl_desc.ptr, n, s.w, s.h, self.d_cand.ptr, stream=stream)
        ctx.encode_tu_batch_dev(src.whole.data_ptr(), self.d_cand.ptr, self.d_cand_recon.ptr, self.d_tu.ptr, n * 66, s.cw, s.ch, self.d_qp.data_ptr(),
                                self.d_iscan.data_ptr(), None, self.d_q.ptr, None, self.d_eob.ptr, None, self.d_dist.ptr, stream=stream)
        ctx.coeff_rate_batch_dev(self.d_tables.data_ptr(), self.d_q.ptr, self.d_eob.ptr, self.d_iscan.data_ptr(), self.d_rd.ptr, n * 66, s.ts_uv, self.d_bits.ptr,
                                 stream=stream)
        ctx.cfl_alpha_decision_batch_dev(self.d_dist.ptr, self.d_bits.ptr, rate_util.tx_scale_shift(s.ts_uv), self.d_alpha_bits.data_ptr(), self.d_job.ptr, n,
                                         self.d_cfl.ptr, stream=stream)
        decisions = self.d_cfl.read(torch, S)[:n]                                # host read 2: the chosen alphas, for their rate
        chosen, _ = mc.apply_cfl_decisions(s, slots, rows, decisions, desc)      # changes s.full["chroma_rate"]
        if len(chosen):
            self.d_cfl_chosen.upload(torch, chosen, S)
            self.d_full.upload(torch, s.full, S)
            ctx.av1_cfl_pred_batch_dev(luma, cb, cr, cb, cr, self.d_cfl_chosen.ptr, len(chosen), s.w, s.h, stream=stream)

    def _cfl_difference(self, inside, mine):
        """the first array the CfL service leaves between its entries (CFL_INSIDE) that is not the restated chain's, as a string, or None"""
        if self.cfl_slots != mine["cfl_slots"]:
            return f"cfl: the service ran on slots {self.cfl_slots}, the restated chain's on {mine['cfl_slots']}"
        for k, what in CFL_INSIDE if self.n_cfl else ():
            g = inside[k]
            w_ = np.ascontiguousarray(mine[k]).reshape(g.shape)
            if not np.array_equal(g, w_):
                rows = np.flatnonzero((g != w_).reshape(len(g), -1).any(axis=1))
                return f"cfl, {what}: tiles {rows[:6].tolist()} differ ({len(rows)} in all; tile = (block * 2 + plane) * 33 + alpha + 16)"
        return None

    def calls(self, ctx, stream):
        """the eight steps of the chain, in order (STAGES), each enqueueing on `stream` (None: the context's own)"""
        s, pl = self.s, self.planes

        def search():
            if s.ifs:
                ctx.md_interp_filter_search_batch_dev(self.refs[0], self.refs[1], pl["src"].arg, self.d_pu.ptr, self.d_ifs_desc.ptr, s.n_search, s.w, s.h,
                                                      1 if s.ifs == "fast" else 2, 1, mc.QUANTIZER, 1, self.d_ifs.ptr, stream=stream)

        def intra():
            for p, (d, n, ts) in enumerate(self.d_intra):
                ctx.av1_intra_pred_batch_dev(pl["nb"].dev[p].data_ptr(), pl["pool"].dev[p].data_ptr(), d.ptr, n, ts, None, None, stream)

        return [search,
                lambda: ctx.av1_inter_pred_batch_dev(self.refs[0], self.refs[1], pl["pool"].arg, self.d_pu.ptr, len(s.pu), s.w, s.h, stream=stream),
                intra,
                lambda: ctx.md_fast_cost_batch_dev(pl["src"].arg, pl["pool"].arg, self.d_fast.ptr, s.n_cand, s.w, s.h, self.d_fast_result.ptr, stream=stream),
                lambda: ctx.md_fast_pick_batch_dev(self.d_fast_result.ptr, self.d_fast.ptr, s.n_cand, self.d_group.ptr, s.n_groups, self.d_pick.ptr, stream=stream),
                lambda: self._full_loop(ctx, fu.LUMA, stream),
                lambda: self._cfl_service(ctx, stream),
                lambda: self._full_loop(ctx, fu.CHROMA | fu.DECIDE, stream)]

    def check(self):
        """after the wait: everything downloaded once and compared in chain order; the first stage that differs is named"""
        s, name = self.s, self.name
        wide = {k: p.download() for k, p in self.planes.items()}                  # asserts every surrounding from the widened planes on
        for k, planes in wide.items():
            for i, (q, h) in enumerate(zip(planes, self.host[k])):
                assert (q[:, h.shape[1]:] == PAD).all(), f"size {name}: wrote right of plane {i} of the {k} planes, in columns {h.shape[1]} .. {q.shape[1] - 1}"
        down = {k: [q[:, :h.shape[1]] for q, h in zip(planes, self.host[k])] for k, planes in wide.items()}
        n, npx = self.n_cfl, s.cw * s.ch
        got = {"ifs": self.d_ifs.get("the search results"), "pu": self.d_pu.get("the PU descriptors"), "pool_luma": down["pool"][:1],
               "fast": self.d_fast_result.get("the fast results"), "picks": self.d_pick.get("the picks"), "slot_luma": down["slot"][:1],
               "cfl": self.d_cfl.get("the alpha decisions", n)[:n], "pool_chroma": down["pool"][1:], "result": self.d_result.get("the full-loop results"),
               "decision": self.d_decision.get("the decisions"), "recon": down["recon"]}
        inside = {k: a.get(what, n * 66)[:n * 66] for (k, what), a in zip(CFL_INSIDE, (self.d_cand, self.d_cand_recon, self.d_q, self.d_eob, self.d_dist, self.d_bits))}
        assert (self.d_work.cpu().numpy()[self.work_bytes:] == GUARD).all(), "wrote behind the workspace"
        _, mine = mc.chain_of(name, self.oracle)
        # in chain order: the stages in front of the CfL service, what the service leaves between its entries, its decisions and the rest
        before = mc.STAGES[:mc.STAGES.index("cfl")]
        diff = mc.first_difference(got, self.want, only=before) or self._cfl_difference(inside, mine) or mc.first_difference(got, self.want)
        if diff is not None:
            diff += "; against the restated chain: " + str(mc.first_difference(got, mine))
        assert diff is None, f"size {name}: the device chain differs from the fixture's at {diff}"
        assert mc.first_difference(got, mine) is None
        assert all(np.array_equal(a, b) for a, b in zip(down["slot"], mine["slot"])), "the slot pool's chroma differs"
        changed = [k for k in self.pu0.dtype.names if k != "interp_filters" and not np.array_equal(got["pu"][k], self.pu0[k])]
        assert not changed, ("descriptor fields other than interp_filters changed", changed)
        for k in ("src", "ref0", "ref1", "nb"):
            assert all(np.array_equal(a, b) for a, b in zip(down[k], self.host[k])), f"the {k} planes were written"
        assert np.array_equal(self.d_fast.get("d_fast"), self.fast0), "d_fast was written"
        assert np.array_equal(self.d_group.get("d_group"), s.groups), "d_group was written"
        assert np.array_equal(self.d_qp.cpu().numpy().view(np.int16).reshape(self.sh["qparams"].shape), self.sh["qparams"]), "d_qparams was written"
        assert np.array_equal(self.d_full.get("d_full"), mine["full"]), "d_full is not what the host uploaded"
        for (d, _, _), p in zip(self.d_intra, range(3)):
            d.get(f"the intra descriptors of plane {p}")
        self.d_ifs_desc.get("the search descriptors")


def _refused(ctx, n):
    if n:
        with pytest.raises(svtav1_hip.SvtHipError, match=rf"{BAD}: {n} PU\(s\) or unit\(s\) refused"):
            ctx.inter_pred_refused()
    assert ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("name", mc.CHAIN_SIZES)
def test_chain_on_the_context_stream(hip_ctx, oracle, name):
    """the five sizes on the context's own stream, the bases 1, 2 or 3 bytes into their buffers at odd strides"""
    torch = pytest.importorskip("torch")
    hip_ctx.inter_pred_refused()
    D = DevChain(torch, oracle, name, shift=1 + mc.CHAIN_SIZES.index(name) % 3)
    for call in D.calls(hip_ctx, None):
        call()
    hip_ctx.synchronize()
    D.check()
    assert hip_ctx.inter_pred_refused() == 0


def _chain_on_a_caller_stream(torch, ctx, oracle, name, busy):
    """the chain of size `name` on a new stream with the host waiting on that stream alone.  busy == "caller": the caller's stream is
    held busy in front of the chain, so work that went elsewhere runs before the stage it depends on; busy == "context": the context's
    own stream is, so work that went there has not run when the caller's stream is through and the results are read"""
    D = DevChain(torch, oracle, name)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())          # stream order behind the uploads, not a host wait
    keep = _gate(torch, s if busy == "caller" else torch.cuda.ExternalStream(ctx.stream), GATE_STEPS[busy])
    for call in D.calls(ctx, s.cuda_stream):
        call()
    s.synchronize()
    try:
        D.check()
        assert ctx.inter_pred_refused() == 0
    finally:
        if busy == "context":
            ctx.synchronize()                            # only now, for the tests that follow: the busy work on the context's stream
    del keep


@pytest.mark.parametrize("name", ["8x8", "16x16", "64x64"])
def test_chain_on_a_caller_stream(hip_ctx, oracle, name):
    """every call takes the caller's stream and the host waits on that stream alone, for its two reads too: nothing of the chain may be
    on the context's own.  The caller's stream busy first: the context's scratch was then last used on a stream other than the
    context's"""
    torch = pytest.importorskip("torch")
    hip_ctx.inter_pred_refused()
    for busy in ("caller", "context"):
        _chain_on_a_caller_stream(torch, hip_ctx, oracle, name, busy)


def test_two_sizes_interleaved_on_one_context(oracle):
    """8x8 on one stream, held back by busy work, and 64x64 on another, alternating call by call on one fresh context: the filter search
    of 64x64 grows the context's trial-tile and job slots while 8x8's work on them is pending, and both chains count into one refusal
    counter.  Then 32x8 on the context's own stream of the same context"""
    torch = pytest.importorskip("torch")
    ctx = svtav1_hip.Context(0)
    try:
        A, B, Cc = DevChain(torch, oracle, "8x8"), DevChain(torch, oracle, "64x64"), DevChain(torch, oracle, "32x8")
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        s2.wait_stream(torch.cuda.current_stream())
        keep = _gate(torch, s1, GATE_STEPS["caller"])    # 8x8 starts late: 64x64 runs ahead wherever the context does not order it behind
        calls_a, calls_b = A.calls(ctx, s1.cuda_stream), B.calls(ctx, s2.cuda_stream)
        assert len(calls_a) == len(calls_b) == len(STAGES)
        for call_a, call_b in zip(calls_a, calls_b):
            call_a()
            call_b()
        s1.synchronize()
        s2.synchronize()
        A.check()
        B.check()
        assert ctx.inter_pred_refused() == 0
        for call in Cc.calls(ctx, None):
            call()
        ctx.synchronize()
        Cc.check()
        assert ctx.inter_pred_refused() == 0
        del keep
    finally:
        ctx.close()


def test_refusals_add_up_along_the_chain(hip_ctx, oracle):
    """4x16 with one BI_PRED PU whose chroma goes sub-8x8 (the prediction refuses it, its tile keeps the pool's fill and the fast loop
    measures that fill) and one group with buffer_total_count = 0 (the pick refuses it, and the full loop again): every array is what the
    restatement says, one query after the chain raises with the sum, a second returns 0"""
    torch = pytest.importorskip("torch")
    name = "4x16_refusals"
    s, mine = mc.chain_of(name, oracle)
    r = mine["refused"]
    assert (r["inter"], r["pick"], r["full"]) == (1, 1, 1) and mc.total_refused(mine) == 3
    f = s.fast[s.refused_pu_row]
    assert (mine["pool_luma"][0][int(f["pred_y"]):int(f["pred_y"]) + s.h, int(f["pred_x"]):int(f["pred_x"]) + s.w] == mc.POOL_FILL).all()
    hip_ctx.inter_pred_refused()
    D = DevChain(torch, oracle, name)
    for call in D.calls(hip_ctx, None):
        call()
    hip_ctx.synchronize()
    D.check()
    _refused(hip_ctx, mc.total_refused(mine))
