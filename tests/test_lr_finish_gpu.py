"""GPU: svthip_rest_finish_search_dev against tests/golden/lr_finish.npz (the reference's own rest_finish_search): every constructed case and
every setting of the chain pictures' tables, all outputs bit-identical (cost by bit pattern).  Every output array lies between guard
elements and is pre-filled with a sentinel, so an element left unwritten or written outside the plane range shows.  Then the refusals:
before launch with the error text set and nothing written, and on the device for a unit out of range, counted by the context."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import lr_finish_util as fu  # noqa: E402
import post_filter_chain_util as pc  # noqa: E402
import svtav1_hip  # noqa: E402
from lr_gpu_util import _ready  # noqa: E402
from test_cdef_gpu import Table  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL8, SENTINEL64 = 0x5A, 0x5A5A5A5A5A5A5A5A
RESULT_WORDS = 13          # svthip_rest_finish_result in int64


class DevTables:
    """one set of search tables on the device with sentinel-filled outputs"""

    def __init__(self, torch, unit_base, tables):
        n = self.n = int(unit_base[3])
        self.unit_base = [int(v) for v in unit_base]
        self.inputs = [Table(torch, a.size, dt, 0x33, a) for a, dt in zip(tables, (np.int64, np.int16, np.int64, np.int32))]
        self.host = [np.ascontiguousarray(a, dt) for a, dt in zip(tables, (np.int64, np.int16, np.int64, np.int32))]
        self.unit_type, self.best = Table(torch, n, np.uint8, SENTINEL8), Table(torch, 4 * n, np.uint8, SENTINEL8)
        self.result = Table(torch, 3 * RESULT_WORDS, np.int64, SENTINEL64)

    def call(self, ctx, rates, plane_range=(0, 3), best=True, stream=None):
        ctx.rest_finish_search_dev(rates, self.unit_base, plane_range[0], plane_range[1], *[t.ptr for t in self.inputs], self.unit_type.ptr,
                                   self.result.ptr, d_best_rtype=self.best.ptr if best else None, stream=stream)

    def get(self):
        """the outputs by the names of lr_finish_util.OUTPUT_KEYS (asserts the guard elements), raw sentinels where nothing was written"""
        res = self.result.get().view(svtav1_hip.rest_finish_result_dtype())
        out = {"unit_type": self.unit_type.get(), "best_rtype": self.best.get().reshape(-1, 4)}
        out.update({k: res[k] for k in fu.RESULT_KEYS})
        return out, res

    def untouched(self, plane_range=(0, 0)):
        """the sentinels of everything outside the plane range survive, and the inputs are what was uploaded"""
        got, res = self.get()
        ps, pe = plane_range
        keep = np.ones(self.n, bool)
        keep[self.unit_base[ps]:self.unit_base[pe]] = False
        raw = res.view(np.int64).reshape(3, RESULT_WORDS)
        return bool((got["unit_type"][keep] == SENTINEL8).all() and (got["best_rtype"][keep] == SENTINEL8).all()
                    and all((raw[p] == SENTINEL64).all() for p in range(3) if not ps <= p < pe)
                    and all(np.array_equal(t.get(), h.reshape(-1)) for t, h in zip(self.inputs, self.host)))


def test_every_fixture_case_is_bit_identical(hip_ctx):
    torch = pytest.importorskip("torch")
    cases = [fu.fixture_case(i) for i in range(fu.n_cases())]
    devs = [DevTables(torch, F["unit_base"], [F[k] for k in fu.INPUT_KEYS]) for F in cases]
    _ready(torch)
    for F, D in zip(cases, devs):
        D.call(hip_ctx, F["rates"], F["range"])
    hip_ctx.synchronize()
    assert hip_ctx.inter_pred_refused() == 0
    for F, D in zip(cases, devs):
        got, _ = D.get()
        diff = fu.first_difference(got, F, F["range"], F["unit_base"])
        assert diff is None, f"case {F['name']}: {diff}"
        assert D.untouched(F["range"]), f"case {F['name']}: something outside planes {F['range']} was written, or an input was"
    assert any(F["range"] == (1, 2) for F in cases)


@pytest.mark.parametrize("name", ("A", "B", "C"))
def test_chain_tables_under_every_setting(hip_ctx, name):
    """the decision alone on the chain fixture's own tables, on a caller's stream"""
    torch = pytest.importorskip("torch")
    want = pc.expected(name)
    base = pc.lu.picture_units(pc.W, pc.H)[1]
    s = torch.cuda.Stream()
    settings = fu.chain_settings(name)
    devs = [DevTables(torch, base, [want[k] for k in fu.INPUT_KEYS]) for _ in settings]
    _ready(torch)
    for k, D in enumerate(devs):
        D.call(hip_ctx, fu.chain_case(name, k)["rates"], best=k % 2 == 0, stream=s.cuda_stream)
    s.synchronize()
    assert hip_ctx.inter_pred_refused() == 0
    for k, D in enumerate(devs):
        got, _ = D.get()
        F = fu.chain_case(name, k)
        if k % 2:
            assert (got["best_rtype"] == SENTINEL8).all()
            got["best_rtype"] = F["best_rtype"]
        diff = fu.first_difference(got, F)
        assert diff is None, f"picture {name}, setting {settings[k]}: {diff}"


def test_refusals_before_launch_write_nothing(hip_ctx):
    torch = pytest.importorskip("torch")
    F = fu.fixture_case([str(n) for n in fu.fixture()["names"]].index("two_units_chroma"))
    D = DevTables(torch, F["unit_base"], [F[k] for k in fu.INPUT_KEYS])
    _ready(torch)
    base, R = F["unit_base"], F["rates"]
    ins = [t.ptr for t in D.inputs]

    def call(rates=R, unit_base=base, ps=0, pe=3, ins=ins, ut=D.unit_type.ptr, res=D.result.ptr, best=D.best.ptr):
        hip_ctx.rest_finish_search_dev(rates, unit_base, ps, pe, *ins, ut, res, d_best_rtype=best)

    def with_in(i, v):
        return ins[:i] + [v] + ins[i + 1:]

    bad = {"null rates": dict(rates=None), "null unit_base": dict(unit_base=None), "null unit_type": dict(ut=None), "null result": dict(res=None),
           "empty plane range": dict(ps=2, pe=2), "plane range backwards": dict(ps=2, pe=1), "plane_end above 3": dict(ps=0, pe=4),
           "unit_base descends": dict(unit_base=[0, 4, 2, 6]), "a plane in range has no unit": dict(unit_base=[0, 2, 2, 4]),
           "result not 8-byte aligned": dict(res=D.result.ptr + 4), "negative rdmult": dict(rates=dict(R, rdmult=-1)),
           "negative wiener cost": dict(rates=dict(R, wiener_cost=[300, -1])), "negative sgrproj cost": dict(rates=dict(R, sgrproj_cost=[-5, 900])),
           "negative switchable cost": dict(rates=dict(R, switchable_cost=[200, 800, -1300]))}
    for i, k in enumerate(fu.INPUT_KEYS):
        bad["null " + k] = dict(ins=with_in(i, None))
        bad[k + " misaligned"] = dict(ins=with_in(i, ins[i] + (1, 1, 4, 2)[i]))
    for what, kw in bad.items():
        with pytest.raises(svtav1_hip.SvtHipError, match=r": \S") as e:
            call(**kw)
        assert "svthip error" in str(e.value), what
    hip_ctx.synchronize()
    assert D.untouched(), "a refused call wrote something"
    assert hip_ctx.inter_pred_refused() == 0
    # a plane outside the range may have no unit, and d_best_rtype may be null
    call(unit_base=[0, 2, 2, 4], ps=0, pe=1, best=None)
    hip_ctx.synchronize()
    got, _ = D.get()
    assert np.array_equal(got["unit_type"][:2], F["unit_type"][:2]) and got["frame_type"][0] == F["frame_type"][0]
    assert (got["best_rtype"] == SENTINEL8).all() and D.untouched((0, 1))


def test_a_unit_out_of_range_is_refused_on_the_device(hip_ctx):
    """an xqd below its range in the second chunk of a 300-unit luma plane: counted once, the plane NONE with zeros, the others as they were"""
    torch = pytest.importorskip("torch")
    F = fu.fixture_case([str(n) for n in fu.fixture()["names"]].index("many_units"))
    tables = [F[k].copy() for k in fu.INPUT_KEYS]
    tables[3][290, 2] = fu.PRJ_MIN[1] - 1
    base = F["unit_base"]
    D = DevTables(torch, base, tables)
    _ready(torch)
    assert hip_ctx.inter_pred_refused() == 0
    D.call(hip_ctx, F["rates"])
    hip_ctx.synchronize()
    with pytest.raises(svtav1_hip.SvtHipError, match=r": 1 PU\(s\) or unit\(s\) refused"):
        hip_ctx.inter_pred_refused()
    assert hip_ctx.inter_pred_refused() == 0
    got, _ = D.get()
    assert fu.first_difference(got, fu.finish(F["rates"], base, *tables)) is None
    assert got["frame_type"][0] == 0 and got["n_tried"][0] == 0 and not got["unit_type"][:base[1]].any() and not got["best_rtype"][:base[1]].any()
    assert fu.first_difference(got, F, (1, 3), base) is None
