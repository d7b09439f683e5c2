"""GPU: the restoration stage on decisions an encoder would make, on the three pictures of the post-reconstruction chain
(tests/post_filter_chain_util.py; regenerated from their seeds, SHA-256 checked) against tests/golden/lr_finish.npz, which holds the
reference's rest_finish_search on the chain fixture's own search tables under a few rate settings a picture, and the digests of the
reference frame filter's planes under each.

  (a) av1_pick_filter_level_dev ... av1_cdef_frame_dev -> av1_search_wiener_dev, av1_search_sgrproj_dev -> per setting
      rest_finish_search_dev -> av1_lr_filter_frame_dev, every call on one caller's stream with no host wait in between: the decision reads
      the tables the searches left on the device and the filter reads the unit types the decision left there.
  (b) av1_pick_filter_restoration_dev, the same stage in one call per setting, on the CDEF'd / deblocked pair of (a): the same taps,
      parameters, unit types, results and digests.
  (c) picture B is 10-bit: it runs the highbd one-call entry.

After one wait everything is downloaded and compared in chain order; the first stage that differs is named."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import lr_finish_util as fu  # noqa: E402
import post_filter_chain_util as pc  # noqa: E402
import svtav1_hip  # noqa: E402
from lr_gpu_util import Guarded, _ready  # noqa: E402
from test_cdef_gpu import Table  # noqa: E402
from test_post_filter_chain_gpu import DevChain  # noqa: E402

pytestmark = pytest.mark.gpu

BEFORE_RESTORATION = ("levels", "masks", "dbk", "mse", "counted", "cdef_result", "fb_strength", "cdef")
SEARCHES = ("wiener_sse", "taps", "n_trials", "sgrproj", "sgr_sse")


class Decision:
    """the outputs of one setting: unit types, best_rtype, results between guards, and restored planes with a stride of their own"""

    def __init__(self, torch, D, k, own_coefficients):
        n = D.n
        self.unit_type, self.best = Table(torch, n, np.uint8, 0x5A), Table(torch, 4 * n, np.uint8, 0x5A)
        self.result = Table(torch, 39, np.int64, 0x5A5A5A5A5A5A5A5A)
        self.restored = Guarded(torch, [np.full_like(p, 9 + k) for p in D.recon0], D.bd, extra=10 + 2 * k + own_coefficients)
        if own_coefficients:
            self.taps, self.sgrproj = Table(torch, 16 * n, np.int16, -77), Table(torch, 4 * n, np.int32, -77)
            self.work = torch.zeros(svtav1_hip.lr_pick_workspace_bytes(D.w, D.h) // 8 + 1, dtype=torch.int64, device="cuda:0")

    def outputs(self):
        res = self.result.get().view(svtav1_hip.rest_finish_result_dtype())
        out = {"unit_type": self.unit_type.get(), "best_rtype": self.best.get().reshape(-1, 4)}
        out.update({key: res[key] for key in fu.RESULT_KEYS})
        return out


@pytest.mark.parametrize("name", tuple(pc.PICTURES))
def test_restoration_stage_on_the_decisions_of_the_device(hip_ctx, name):
    torch = pytest.importorskip("torch")
    D = DevChain(torch, name)                         # checks the SHA-256 of the regenerated inputs
    settings = fu.chain_settings(name)
    cases = [fu.chain_case(name, k) for k in range(len(settings))]
    base = pc.lu.picture_units(pc.W, pc.H)[1]
    parts = [Decision(torch, D, k, False) for k in range(len(settings))]
    whole = [Decision(torch, D, k, True) for k in range(len(settings))]
    _ready(torch)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())        # stream order behind the uploads, not a host wait
    on = {"bit_depth": D.bd, "stream": s.cuda_stream}
    for call in D.calls(hip_ctx, s.cuda_stream)[:6]:  # pick, deblock, CDEF search, CDEF, Wiener search, self-guided search
        call()
    for F, P in zip(cases, parts):                    # (a)
        hip_ctx.rest_finish_search_dev(F["rates"], base, 0, 3, D.wiener_sse.ptr, D.taps.ptr, D.sgr_sse.ptr, D.sgrproj.ptr, P.unit_type.ptr, P.result.ptr,
                                       d_best_rtype=P.best.ptr, stream=s.cuda_stream)
        hip_ctx.av1_lr_filter_frame_dev(D.lr, P.restored.ptr, P.restored.stride, 0, 3, P.unit_type.ptr, D.taps.ptr, D.sgrproj.ptr, **on)
    for F, P in zip(cases, whole):                    # (b), (c)
        hip_ctx.av1_pick_filter_restoration_dev(D.lr, F["rates"], P.work.data_ptr(), P.restored.ptr, P.restored.stride, P.unit_type.ptr, P.taps.ptr,
                                                P.sgrproj.ptr, P.result.ptr, **on)
    s.synchronize()
    assert hip_ctx.inter_pred_refused() == 0          # waits on the stream of the last restoration call, the caller's

    planes = {k: g.planes() for k, g in (("recon", D.recon), ("cdef", D.cdef))}
    got = {"dbk": planes["recon"][0], "cdef": planes["cdef"][0]}
    for k, t in (("levels", D.levels), ("masks", D.masks), ("mse", D.mse), ("counted", D.counted), ("cdef_result", D.result), ("fb_strength", D.fbs),
                 ("wiener_sse", D.wiener_sse), ("taps", D.taps), ("n_trials", D.n_trials), ("sgrproj", D.sgrproj), ("sgr_sse", D.sgr_sse)):
        got[k] = t.get()
    diff = pc.first_difference(got, D.want, only=BEFORE_RESTORATION + SEARCHES)
    assert diff is None, f"picture {name}: the device chain differs from the reference's at {diff}"
    assert int(D.pending.get()[0]) == 0, "the Wiener search left walks pending"
    for k, (F, P, W) in enumerate(zip(cases, parts, whole)):
        at = f"picture {name}, setting {settings[k]}"
        diff = fu.first_difference(P.outputs(), F)
        assert diff is None, f"{at}: the decision of the separate entries differs at {diff}"
        restored, guard_ok = P.restored.planes()
        assert guard_ok, f"{at}: a sample outside the restored planes was written"
        assert pc.plane_digest(restored)[0] == F["digest_restored"][0], f"{at}: restoration on the device's decision: the digest of the three planes differs"
        one = W.outputs()
        assert (one["best_rtype"] == 0x5A).all()      # the one-call entry keeps no best_rtype
        one["best_rtype"] = F["best_rtype"]
        for key, t in (("taps", W.taps), ("sgrproj", W.sgrproj)):
            assert np.array_equal(t.get(), np.asarray(D.want[key]).reshape(-1)), f"{at}: the one-call entry's {key} differ"
        diff = fu.first_difference(one, F)
        assert diff is None, f"{at}: the decision of the one-call entry differs at {diff}"
        restored1, guard_ok = W.restored.planes()
        assert guard_ok and all(np.array_equal(a, b) for a, b in zip(restored1, restored)), f"{at}: the one-call entry's planes are not those of the parts"
    assert all(g[1] for g in planes.values()), "a sample outside the chain's planes was written"
    assert all(np.array_equal(a, b) for a, b in zip(D.source.planes()[0], D.source0)), "the source planes were written"
