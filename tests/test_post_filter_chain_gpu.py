"""GPU: the post-reconstruction entries as the chain they were built to be, against tests/golden/post_filter_chain.npz (the reference's own
stages run as a chain on three 200 x 200 pictures; tests/post_filter_chain_util.py).

  av1_pick_filter_level_dev -> av1_loop_filter_frame_dev (the levels stay in d_levels) -> av1_cdef_search_dev -> av1_cdef_frame_dev ->
  av1_search_wiener_dev, av1_search_sgrproj_dev (on the CDEF'd / deblocked pair the device itself made) -> av1_lr_filter_frame_dev (taps
  and parameters straight from the searches, unit types u % 3) -> [highbd_]add_film_grain_dev (one-call form, tables in context scratch)

One set of guarded buffers per picture: the reconstruction (deblocked in place), the source, the CDEF, restoration and grain outputs, each
with a stride of its own, so every hand-over is between buffers of different strides.  Between the first call and the last there is no
host synchronisation, no download and no Python-side read; after one wait everything is downloaded and compared in chain order, and the
first stage that differs is named.  The chain runs on the context's stream, on a caller's stream (the host waits on that stream only), and
as two pictures of different bit depths interleaved call by call on two streams of one context, which share the context's film-grain
table slot and refusal counter.

The caller-stream test runs the chain twice, with device work enqueued in front of it (_gate) while the host enqueues the calls: once on
the caller's stream, so that a launch that went to another stream runs before the stage it depends on, and once on the context's own
stream, so that a launch or a memset that went there has not run when the results are read.  The busy work can only make a misplaced
launch visible, it cannot fail a correct run; where the runtime puts both streams on one hardware queue they run in the order of their
calls and it shows nothing.  A tensor that torch fills is handed to an entry only after _ready() (tests/lr_gpu_util.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import cdef_util as cu  # noqa: E402
import film_grain_util as fu  # noqa: E402
import lr_util as lu  # noqa: E402
import post_filter_chain_util as pc  # noqa: E402
import svtav1_hip  # noqa: E402
from lr_gpu_util import Guarded, _dev, _ready  # noqa: E402
from test_cdef_gpu import SKIP_GUARD, Table  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = tuple(pc.PICTURES)
STAGES = ("pick", "deblock", "cdef search", "cdef frame", "wiener search", "sgrproj search", "restoration", "grain")
# Elementwise passes over 128 MB that keep a stream busy.  In front of the chain on the caller's stream they have to outlast the host's
# enqueueing of the calls; on the context's stream they have to outlast the whole chain on the caller's stream.
GATE_STEPS = {"caller": 100, "context": 600}


def _gate(torch, s, steps):
    """`steps` passes of elementwise work on `s`, enqueued in a fraction of the time they run: returns the tensor they work on, to be kept
    until the wait"""
    a = torch.zeros(1 << 25, dtype=torch.float32, device="cuda:0")
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(steps):
            a.mul_(1.0001).add_(1.0)
    return a


class DevChain:
    """one picture on the device with every buffer and array of the chain, and the chain as a list of calls"""

    def __init__(self, torch, name):
        self.torch, self.name = torch, name
        P = self.P = pc.PICTURES[name]
        self.bd, self.w, self.h = P["bd"], pc.W, pc.H
        self.mi, self.recon0, self.source0 = pc.make_picture(name)
        self.want = pc.expected(name, self.recon0)
        for k, v in pc.input_digests(self.mi, self.recon0, self.source0).items():
            assert np.array_equal(v, self.want["sha256_" + k]), f"picture {name}: the regenerated {k} is not the fixture's input"
        blank = lambda v: [np.full_like(p, v) for p in self.recon0]  # noqa: E731
        self.recon, self.source = Guarded(torch, self.recon0, self.bd), Guarded(torch, self.source0, self.bd, extra=2)
        self.cdef, self.restored, self.grain = (Guarded(torch, blank(7 + k), self.bd, extra=4 + 2 * k) for k in range(3))
        assert all(len({g.stride[p] for g in self.buffers().values()}) == 5 for p in range(3))
        self.d_mi = _dev(torch, self.mi)
        skip = pc.skip_map(self.mi)
        sk = np.ones((skip.shape[0] + 2, skip.shape[1] + SKIP_GUARD), np.uint8)
        sk[1:-1, 1:1 + skip.shape[1]] = skip
        self.skip_host, self.d_skip = sk, _dev(torch, sk)
        nh, nv = cu.geometry(self.w, self.h)
        nfb = self.nfb = nh * nv
        self.n = n = lu.picture_units(self.w, self.h)[1][3]
        T = lambda count, dt, fill, host=None: Table(torch, count, dt, fill, host)  # noqa: E731
        self.levels, self.sse_tables, self.masks = T(4, np.int32, -77), T(5 * 64, np.uint64, 0x5A5A5A5A5A5A5A5A), T(5, np.uint64, 0x5A5A5A5A5A5A5A5A)
        self.mse, self.counted = T(2 * nfb * 64, np.uint64, 0x5A5A5A5A5A5A5A5A), T(nfb, np.uint8, 0x5A)
        self.result, self.fbs = T(21, np.int32, -77), T(nfb, np.int8, 0x5A)
        self.wiener_sse, self.taps, self.n_trials = T(2 * n, np.int64, -77), T(16 * n, np.int16, -77), T(n, np.int32, -77)
        # pending sits alone: av1_search_wiener_dev clears it with a 4-byte memset
        self.pending = T(1, np.int32, -77)
        self.sgrproj, self.sgr_sse = T(4 * n, np.int32, -77), T(n, np.int64, -77)
        self.unit_type = T(n, np.uint8, 0x5A, self.want["unit_type"])
        self.work_wiener = torch.zeros(svtav1_hip.lr_workspace_bytes(n) // 8 + 1, dtype=torch.int64, device="cuda:0")
        self.work_sgr = torch.zeros(svtav1_hip.sgrproj_workspace_bytes(self.w, self.h) // 8 + 1, dtype=torch.int64, device="cuda:0")
        w, h = self.w, self.h
        self.lf = svtav1_hip.make_lf_picture(w, h, self.recon.ptr, self.recon.stride, self.source.ptr, self.source.stride)
        self.cdef_pic = svtav1_hip.make_cdef_picture(w, h, self.recon.ptr, self.recon.stride, self.d_skip.data_ptr() + sk.shape[1] + 1, sk.shape[1],
                                                     self.source.ptr, self.source.stride, self.cdef.ptr, self.cdef.stride)
        self.lr = svtav1_hip.make_lr_picture(w, h, self.cdef.ptr, self.cdef.stride, self.recon.ptr, self.recon.stride, self.source.ptr, self.source.stride)
        self.grain_params = svtav1_hip.film_grain_params(**fu.PARAM_SETS[P["grain_set"]])
        _ready(torch)

    def buffers(self):
        return {"recon": self.recon, "source": self.source, "cdef": self.cdef, "restored": self.restored, "grain": self.grain}

    def calls(self, ctx, stream):
        """the eight calls of the chain, in order (STAGES), each enqueueing on `stream` (None: the context's own)"""
        bd, q, mi, ms = self.bd, self.P["base_qindex"], self.d_mi.data_ptr(), self.mi.shape[1]
        on = {"bit_depth": bd, "stream": stream}

        def grain():
            a = (self.grain_params, self.restored.ptr, self.restored.stride, self.grain.ptr, self.grain.stride, self.w, self.h)
            if bd == 8:
                ctx.add_film_grain_dev(*a, d_tables=None, stream=stream)
            else:
                ctx.highbd_add_film_grain_dev(*a, bd, d_tables=None, stream=stream)

        return [lambda: ctx.av1_pick_filter_level_dev(self.lf, mi, ms, self.P["last_levels"], 0, 0, self.levels.ptr, self.sse_tables.ptr, self.masks.ptr, **on),
                lambda: ctx.av1_loop_filter_frame_dev(self.lf, mi, ms, self.levels.ptr, 0, 0, 3, **on),
                lambda: ctx.av1_cdef_search_dev(self.cdef_pic, q, self.mse.ptr, self.counted.ptr, self.result.ptr, self.fbs.ptr, **on),
                lambda: ctx.av1_cdef_frame_dev(self.cdef_pic, self.result.ptr, self.fbs.ptr, 0, 3, **on),
                lambda: ctx.av1_search_wiener_dev(self.lr, 0, 3, self.work_wiener.data_ptr(), self.wiener_sse.ptr, self.taps.ptr, self.n_trials.ptr,
                                                  self.pending.ptr, n_steps=0, **on),
                lambda: ctx.av1_search_sgrproj_dev(self.lr, 0, 3, self.work_sgr.data_ptr(), self.sgrproj.ptr, self.sgr_sse.ptr, None, **on),
                lambda: ctx.av1_lr_filter_frame_dev(self.lr, self.restored.ptr, self.restored.stride, 0, 3, self.unit_type.ptr, self.taps.ptr,
                                                    self.sgrproj.ptr, **on),
                grain]

    def check(self):
        """after the wait: everything downloaded and compared in chain order; the first stage that differs is named"""
        planes = {k: g.planes() for k, g in self.buffers().items()}
        got = {"dbk": planes["recon"][0], "cdef": planes["cdef"][0], "restored": planes["restored"][0], "grain": planes["grain"][0]}
        for k, t in (("levels", self.levels), ("masks", self.masks), ("mse", self.mse), ("counted", self.counted), ("cdef_result", self.result),
                     ("fb_strength", self.fbs), ("wiener_sse", self.wiener_sse), ("taps", self.taps), ("n_trials", self.n_trials),
                     ("sgrproj", self.sgrproj), ("sgr_sse", self.sgr_sse), ("unit_type", self.unit_type)):
            got[k] = t.get()          # asserts the guard elements of the array
        diff = pc.first_difference(got, self.want)
        if diff is not None and "dbk" not in self.want:     # digests only: the restated chain shows where
            diff += "; against the restated chain: " + str(pc.first_difference(got, pc.chain_of(self.name)[3]))
        assert diff is None, f"picture {self.name}: the device chain differs from the reference's at {diff}"
        for k, (_, guard_ok) in planes.items():
            assert guard_ok, f"picture {self.name}: a sample outside the {k} planes was written"
        assert all(np.array_equal(a, b) for a, b in zip(planes["source"][0], self.source0)), "the source planes were written"
        assert np.array_equal(self.d_skip.cpu().numpy().reshape(self.skip_host.shape), self.skip_host), "the skip map was written"
        assert np.array_equal(self.d_mi.cpu().numpy().view(self.mi.dtype).reshape(self.mi.shape), self.mi), "the mode-info grid was written"
        assert int(self.pending.get()[0]) == 0, "the Wiener search left walks pending"
        self.sse_tables.get()


@pytest.mark.parametrize("name", NAMES)
def test_chain_on_the_context_stream(hip_ctx, name):
    torch = pytest.importorskip("torch")
    D = DevChain(torch, name)
    for call in D.calls(hip_ctx, None):
        call()
    hip_ctx.synchronize()
    D.check()
    assert hip_ctx.inter_pred_refused() == 0


def _chain_on_a_caller_stream(torch, ctx, name, busy, s=None):
    """the chain of picture `name` on a new stream with the host waiting on that stream alone.  busy == "caller": the caller's stream is
    held busy in front of the chain, so work that went elsewhere runs before the stage it depends on; busy == "context": the context's
    own stream is, so work that went there has not run when the caller's stream is through and the results are read"""
    D = DevChain(torch, name)
    s = s or torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())          # stream order behind the uploads, not a host wait
    keep = _gate(torch, s if busy == "caller" else torch.cuda.ExternalStream(ctx.stream), GATE_STEPS[busy])
    for call in D.calls(ctx, s.cuda_stream):
        call()
    s.synchronize()
    try:
        D.check()
        assert ctx.inter_pred_refused() == 0             # waits on the stream of the last restoration call, the caller's
    finally:
        if busy == "context":
            ctx.synchronize()                            # only now, for the tests that follow: the busy work on the context's stream
    del keep


@pytest.mark.parametrize("name", NAMES)
def test_chain_on_a_caller_stream(hip_ctx, name):
    """every call takes the caller's stream and the host waits on that stream alone: nothing of the chain may be on the context's own.
    The caller's stream busy first: the context's scratch was then last used on a stream other than the context's, and the second
    run's stream does not have to order itself behind the busy context stream"""
    torch = pytest.importorskip("torch")
    for busy in ("caller", "context"):
        _chain_on_a_caller_stream(torch, hip_ctx, name, busy)


def test_two_pictures_interleaved_on_one_context():
    """A (8 bits, grain set 4) on one stream and B (10 bits, grain set 5) on another, alternating call by call on one fresh context: the
    one-call grain form builds both table blocks in the same context slot and the restoration filter counts refusals in the same counter.
    Then C on the context's own stream of the same context"""
    torch = pytest.importorskip("torch")
    ctx = svtav1_hip.Context(0)
    try:
        A, B, Cc = DevChain(torch, "A"), DevChain(torch, "B"), DevChain(torch, "C")
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        s2.wait_stream(torch.cuda.current_stream())
        keep = _gate(torch, s1, GATE_STEPS["caller"])    # A starts late: B runs ahead wherever the context does not order it behind A
        calls_a, calls_b = A.calls(ctx, s1.cuda_stream), B.calls(ctx, s2.cuda_stream)
        assert len(calls_a) == len(calls_b) == len(STAGES)
        for call_a, call_b in zip(calls_a, calls_b):     # A.pick, B.pick, A.deblock, B.deblock, ... A.grain, B.grain
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
