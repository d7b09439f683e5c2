"""GPU: the state a svthip_ctx carries from one call to the next, each test on contexts of its own.

A context keeps grow-only scratch slots, the SB-origin table of the host-pointer picture forms (slot 9, SLOT_SB_TABLE in
svthip_glue.h's `enum Slot`, whose order gives the slot numbers quoted here; rebuilt when the geometry changes), the stream that last used its scratch, and the inter-prediction refusal counter.  Every other GPU test shares one session
context in a fixed order, so none of them sees a call that follows a different one: another geometry, PU count, list count or stream,
or an svthip_reserve.  Here every step of such sequences is compared bit-exactly with the oracle (the numpy restatement for inter
prediction); expected results are computed once per (pictures, geometry, PU count, list count) and reused by every step that repeats
that input.

Pictures: A = 640 x 360 (10 x 6 SBs, partial last SB row), B = 832 x 480 (13 x 8 SBs), textured (synth.synth_luma) so that a wrong SB
origin gives wrong vectors.  The 3840 x 2160 reserve really reallocates slot 9 after a picture at A: see _slot9_bytes."""
import ctypes as C

import numpy as np
import pytest

import inter_pred_util as ipu
import svtav1_hip
from me_chain_util import compare_results, oracle_me_picture
from svtav1_hip import synth
from tq_util import oracle_encode_batch, random_encode_batch

pytestmark = pytest.mark.gpu

A, B, BIG = (640, 360), (832, 480), (3840, 2160)
OIS_ORDER = ["slice_is_intra", "temporal_layer_index", "is_used_as_reference_flag", "input_resolution_4k", "limit_ois_to_dc_mode_flag",
             "cu8x8_mode", "enc_mode"]
OIS_GENERAL = dict(temporal_layer_index=2, is_used_as_reference_flag=1)   # reads the ME distortions
OIS_INTRA = dict(slice_is_intra=1)                                        # reads no ME rows


def _n_sb(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def _slot9_bytes(w, h):
    """what ensure_scratch allocates for the SB-origin table of a first picture at w x h (4-byte origins, 1/4 + 4096 bytes of slack)"""
    n = 4 * _n_sb(w, h)
    return n + n // 4 + 4096


def _ois_params(kw):
    p = svtav1_hip.OisParams()
    for k, v in kw.items():
        setattr(p, k, v)
    return p, np.array([kw.get(k, 0) for k in OIS_ORDER], np.int32)


class Expected:
    """The oracle's answers, each computed on first use."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.pics = {g: [synth.PaPicture(synth.synth_luma(g[0], g[1], t)) for t in (3, 0, 7)] for g in (A, B)}
        self._me, self._ois = {}, {}

    def params(self, geo, two_lists):
        return svtav1_hip.default_me_params(geo[0], geo[1], 3, 1 if two_lists else 0)

    def me(self, geo, two_lists, n_pu):
        k = (geo, two_lists, n_pu)
        if k not in self._me:
            self._me[k] = oracle_me_picture(self.oracle, self.pics[geo], self.params(geo, two_lists), two_lists, True, 0, n_pu=n_pu)[0]
        return self._me[k]

    def ois(self, geo, me_key=None):
        """me_key None: the intra branch; else (two_lists, n_pu) of the ME rows the general branch reads"""
        k = (geo, me_key)
        if k not in self._ois:
            _, op = _ois_params(OIS_INTRA if me_key is None else OIS_GENERAL)
            me = None if me_key is None else np.ascontiguousarray(self.me(geo, *me_key)["distortion"][:, :85, 0])
            self._ois[k] = self.oracle.ois_search_picture(self.pics[geo][0].full, 68, geo[0], geo[1], op, me)
        return self._ois[k]


@pytest.fixture(scope="module")
def expected(oracle):
    return Expected(oracle)


def _host(pics):
    return [svtav1_hip.HostPicture(p.full.ctypes.data, p.stride, 68, 68, p.width, p.height) for p in pics]


def _check_me(got, want, step):
    """got: ME_CU_RESULT_DTYPE [n_sb][n_pu]; the message names the step and the SBs that differ"""
    fields = ("totalMeCandidateIndex", "xMvL0", "yMvL0", "xMvL1", "yMvL1", "distortion", "direction")
    bad = sorted({int(i) for f in fields for i in np.argwhere(got[f] != want[f])[:, 0]})
    try:
        compare_results(got, want)
    except AssertionError as e:
        raise AssertionError(f"{step}: SBs {bad[:16]}{' ...' if len(bad) > 16 else ''} of {len(want)} differ from the oracle; {e}") from None


def _check_rows(rows, want, step):
    """rows: MeCuResults_t rows (ME_CU_RESULT_REF_DTYPE) of the host-pointer entry"""
    dd = rows["distortionDirection"]
    got = np.zeros(rows.shape, svtav1_hip.ME_CU_RESULT_DTYPE)
    for f in ("xMvL0", "yMvL0", "xMvL1", "yMvL1", "totalMeCandidateIndex"):
        got[f] = rows[f]
    got["distortion"] = dd["distortion"]
    assert (dd["direction"] < 3).all(), f"{step}: direction words outside 0..2"
    got["direction"] = dd["direction"]
    _check_me(got, want, step)
    assert not rows.view(np.uint8).reshape(rows.shape + (40,))[..., 33:].any(), f"{step}: padding bytes not 0"


def _check_ois(got, want, step):
    for name, g, w in zip(("cand", "total"), got, want):
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{step}: OIS {name}: {len(bad)} mismatches, SBs {sorted(set(bad[:, 0].tolist()))[:16]}"


class HostMe:
    """Host-pointer ME (and OIS) steps of one context, every result checked against the oracle."""

    def __init__(self, ctx, expected, two_lists, n_pu):
        self.ctx, self.x, self.two_lists, self.n_pu = ctx, expected, two_lists, n_pu

    def me(self, geo, step):
        hp = _host(self.x.pics[geo])
        rows = self.ctx.motion_estimate_picture(hp[0], hp[1], hp[2] if self.two_lists else None, self.x.params(geo, self.two_lists), True, 0,
                                                self.n_pu)
        _check_rows(rows, self.x.me(geo, self.two_lists, self.n_pu), f"ME {step}")
        return rows

    def ois(self, geo, rows, step):
        cur = _host(self.x.pics[geo][:1])[0]
        if rows is not None:
            got = self.ctx.open_loop_intra_search_picture(cur, _ois_params(OIS_GENERAL)[0], rows, self.n_pu)
            _check_ois(got, self.x.ois(geo, (self.two_lists, self.n_pu)), f"OIS general {step}")
        got = self.ctx.open_loop_intra_search_picture(cur, _ois_params(OIS_INTRA)[0], None, self.n_pu)
        _check_ois(got, self.x.ois(geo), f"OIS intra {step}")


# -- geometry changes and svthip_reserve between host-pointer picture calls ----------------------------------------------------

RESERVE_SEQUENCE = [(A, "A first"), ("reserve", True), (A, "A after the 4K reserve"), (B, "B after A"), (A, "A after B"), ("reserve", False),
                    (A, "A after the device-form 4K reserve")]


def _run_reserve_sequence(expected, two_lists, n_pu, with_ois):
    assert 4 * _n_sb(*BIG) > _slot9_bytes(*A), "the 4K reserve must reallocate the SB-origin table"
    ctx = svtav1_hip.Context(0)
    try:
        run = HostMe(ctx, expected, two_lists, n_pu)
        for geo, step in RESERVE_SEQUENCE:
            if geo == "reserve":
                ctx.reserve(BIG[0], BIG[1], n_pu, 1, host_forms=step)
                continue
            rows = run.me(geo, step)
            if with_ois:
                if step == RESERVE_SEQUENCE[-1][1]:   # OIS at B straight after ME at A: both entries lay slots 8-11 out differently
                    run.ois(B, rows_b, "B straight after ME at A")
                run.ois(geo, rows, step)
                if geo == B:
                    rows_b = rows
    finally:
        ctx.close()


@pytest.mark.parametrize("n_pu", [85, 209])
@pytest.mark.parametrize("two_lists", [False, True], ids=["P", "B"])
def test_host_me_across_geometries_and_reserve(expected, two_lists, n_pu):
    """A -> reserve(3840, 2160, host_forms) -> A -> B -> A -> reserve(3840, 2160, device forms only) -> A on one context"""
    _run_reserve_sequence(expected, two_lists, n_pu, with_ois=False)


@pytest.mark.parametrize("n_pu", [85, 209])
@pytest.mark.parametrize("two_lists", [False, True], ids=["P", "B"])
def test_host_ois_after_me_across_geometries_and_reserve(expected, two_lists, n_pu):
    """the same sequence with open_loop_intra_search_picture (general branch fed the rows just returned, and the intra branch) after every
    ME step; after the last ME step (at A) OIS runs at B first, straight after ME at A, then at A"""
    _run_reserve_sequence(expected, two_lists, n_pu, with_ois=True)


# -- device-form ME chain ---------------------------------------------------------------------------------------------------

class DevicePictures:
    """device pool and SB table of one geometry's three pictures"""

    def __init__(self, torch, pics):
        pool, self.descs = svtav1_hip.build_picture_pool(pics)
        sb = svtav1_hip.sb_origins(pics[0].width, pics[0].height)
        self.n = sb.shape[0]
        self.d_pool = torch.from_numpy(np.concatenate([pool, np.zeros(64, np.uint8)])).to("cuda:0")
        self.d_sb = torch.from_numpy(sb.view(np.int16).copy()).to("cuda:0")

    def out(self, torch, n_pu):
        return torch.full((self.n, n_pu, 24), 0xA5, dtype=torch.uint8, device="cuda:0")

    def launch(self, ctx, P, two_lists, n_pu, d_out, stream=None):
        d = self.descs
        if n_pu == 209:
            ctx.motion_estimate209_batch_dev(self.d_pool.data_ptr(), [d[0]], [d[1]], [d[2]] if two_lists else None, P, self.d_sb.data_ptr(),
                                             self.n, d_out.data_ptr(), True, 0, stream=stream)
        else:
            ctx.motion_estimate_picture_dev(self.d_pool.data_ptr(), d[0], d[1], d[2] if two_lists else None, P, self.d_sb.data_ptr(), self.n,
                                            d_out.data_ptr(), True, 0, stream=stream)


def _as_results(d_out, n_pu):
    return d_out.cpu().numpy().view(svtav1_hip.ME_CU_RESULT_DTYPE).reshape(-1, n_pu)


def test_device_me_pu_count_and_list_count_changes(expected):
    """motion_estimate_picture_dev / motion_estimate209_batch_dev at one geometry, 85 -> 209 -> 85 PUs and P -> B -> P: the slot-5 layout
    and the slot-7 size depend on both"""
    torch = pytest.importorskip("torch")
    dp = DevicePictures(torch, expected.pics[A])
    seq = [(False, 85), (True, 85), (True, 209), (True, 85), (False, 209), (False, 85), (True, 209)]
    ctx = svtav1_hip.Context(0)
    try:
        for i, (two_lists, n_pu) in enumerate(seq):
            d_out = dp.out(torch, n_pu)
            torch.cuda.synchronize()
            dp.launch(ctx, expected.params(A, two_lists), two_lists, n_pu, d_out)
            ctx.synchronize()
            _check_me(_as_results(d_out, n_pu), expected.me(A, two_lists, n_pu), f"step {i}: {'B' if two_lists else 'P'} {n_pu} PUs")
    finally:
        ctx.close()


def _tq_device(torch, b):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")  # noqa: E731
    n_tu, n = len(b["desc"]), b["n"]
    d = {k: dev(b[k]) for k in ("src", "pred", "desc", "qparams", "iscan")}
    d["recon"] = dev(b["pred"])
    for k in ("coeff", "qcoeff", "dqcoeff"):
        d[k] = torch.full((n_tu * n,), 5, dtype=torch.int32, device="cuda:0")
    d["eob"] = torch.full((n_tu,), -1, dtype=torch.int16, device="cuda:0")
    d["energy"] = torch.full((n_tu,), -1, dtype=torch.int64, device="cuda:0")
    d["dist"] = torch.full((n_tu, 2), -1, dtype=torch.int64, device="cuda:0")
    return d


def _tq_launch(ctx, b, d, stream):
    ctx.encode_tu_batch_dev(d["src"].data_ptr(), d["pred"].data_ptr(), d["recon"].data_ptr(), d["desc"].data_ptr(), len(b["desc"]), b["w"], b["h"],
                            d["qparams"].data_ptr(), d["iscan"].data_ptr(), d["coeff"].data_ptr(), d["qcoeff"].data_ptr(), d["dqcoeff"].data_ptr(),
                            d["eob"].data_ptr(), d["energy"].data_ptr(), d["dist"].data_ptr(), stream=stream)


def _tq_check(d, want, step):
    got = {"recon": d["recon"].cpu().numpy(), "coeff": d["coeff"].cpu().numpy(), "qcoeff": d["qcoeff"].cpu().numpy(),
           "dqcoeff": d["dqcoeff"].cpu().numpy(), "eob": d["eob"].cpu().numpy().view(np.uint16), "energy": d["energy"].cpu().numpy().view(np.uint64),
           "dist": d["dist"].cpu().numpy().view(np.uint64)}
    for k, g in got.items():
        assert np.array_equal(g.reshape(want[k].shape), want[k]), f"{step}: T/Q {k} differs from the oracle"


def _inter_batch(seed, size, n, refused=0):
    """a random whole-PU batch on a 512 x 256 picture and the restatement's prediction; `refused` BI_PRED PUs get sub-8x8 chroma"""
    bw, bh = size
    rng = np.random.default_rng(seed)
    border = ipu.border_for(bw, bh)
    refs = [ipu.random_picture(rng, 512, 256, border, 8, kind) for kind in ("noise", "smooth")]
    desc = ipu.random_descs(rng, n, bw, bh, 512, 256)
    for i in [i for i, d in enumerate(desc) if d["has_uv"]][:refused]:
        desc[i]["pred_direction"] = 2
        desc[i]["nb_is_inter"][:] = 1
    want = _blank_picture(8)
    assert ipu.predict(refs[0], refs[1], want, desc, bw, bh, 8) == refused
    return refs, desc, want


def _blank_picture(bd):
    dt = np.uint8 if bd == 8 else np.uint16
    return ipu.Picture(np.full((256, 512), 0x55, dt), np.full((128, 256), 0x55, dt), np.full((128, 256), 0x55, dt), 0)


class InterDevice:
    def __init__(self, torch, refs, desc, size):
        self.refs, self.desc, self.size = refs, desc, size
        self.d0, self.d1, self.dp = ipu.to_device(refs[0]), ipu.to_device(refs[1]), ipu.to_device(_blank_picture(8))
        self.d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to("cuda:0")

    def launch(self, ctx, stream):
        ctx.av1_inter_pred_batch_dev(ipu.planes_of(self.d0, self.refs[0]), ipu.planes_of(self.d1, self.refs[1]), ipu.planes_of(self.dp, _blank_picture(8)),
                                     self.d_desc.data_ptr(), len(self.desc), self.size[0], self.size[1], stream=stream)

    def check(self, want, step):
        for p in ("y", "cb", "cr"):
            g, w = self.dp[p].cpu().numpy(), getattr(want, p)
            bad = np.argwhere(g != w)
            assert bad.size == 0, f"{step}: inter prediction {p}: {len(bad)} samples differ from the restatement, first at {bad[0]}"


def test_caller_streams_and_growth_in_flight(expected):
    """ME chain at A on s1, then at B on s2 with no host wait (slots 5 and 7 grow while s1 may still run), A on the context's stream, a
    host-pointer call (synchronous, must be ordered behind s2), then fused T/Q and whole-PU inter prediction on s1 and s2; one
    synchronisation at the end"""
    torch = pytest.importorskip("torch")
    dA, dB = DevicePictures(torch, expected.pics[A]), DevicePictures(torch, expected.pics[B])
    outs = {"A on s1": dA.out(torch, 85), "B on s2": dB.out(torch, 85), "A on the context stream": dA.out(torch, 85)}
    tq = [random_encode_batch(np.random.default_rng(61 + i), n, w, h) for i, (n, w, h) in enumerate(((40, 16, 16), (24, 64, 64)))]
    tq_want = [oracle_encode_batch(expected.oracle, b) for b in tq]
    tq_dev = [_tq_device(torch, b) for b in tq]
    ip = [_inter_batch(70 + i, size, 200) for i, size in enumerate(((8, 8), (32, 16)))]
    ip_dev = [InterDevice(torch, refs, desc, size) for (refs, desc, _), size in zip(ip, ((8, 8), (32, 16)))]
    want_me = {"A on s1": expected.me(A, True, 85), "B on s2": expected.me(B, True, 85), "A on the context stream": expected.me(A, True, 85)}
    want_host = expected.me(B, True, 85)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()   # every input and output buffer is ready before the first call
    ctx = svtav1_hip.Context(0)
    try:
        dA.launch(ctx, expected.params(A, True), True, 85, outs["A on s1"], stream=s1.cuda_stream)
        dB.launch(ctx, expected.params(B, True), True, 85, outs["B on s2"], stream=s2.cuda_stream)
        dA.launch(ctx, expected.params(A, True), True, 85, outs["A on the context stream"])
        hp = _host(expected.pics[B])
        rows = ctx.motion_estimate_picture(hp[0], hp[1], hp[2], expected.params(B, True), True, 0, 85)
        for (b, d), s in zip(zip(tq, tq_dev), (s1, s2)):
            _tq_launch(ctx, b, d, s.cuda_stream)
        for d, s in zip(ip_dev, (s1, s2)):
            d.launch(ctx, s.cuda_stream)
        torch.cuda.synchronize()
        _check_rows(rows, want_host, "host-pointer ME at B after the stream calls")
        for k, d_out in outs.items():
            _check_me(_as_results(d_out, 85), want_me[k], k)
        for i, (d, w) in enumerate(zip(tq_dev, tq_want)):
            _tq_check(d, w, f"T/Q batch {i} on s{i + 1}")
        for i, (d, (_, _, w)) in enumerate(zip(ip_dev, ip)):
            d.check(w, f"inter prediction batch {i} on s{i + 1}")
        assert ctx.inter_pred_refused() == 0
    finally:
        ctx.close()


# -- the refusal counter of whole-PU inter prediction across streams ---------------------------------------------------------------

def test_refusal_counter_across_streams():
    """one refused BI_PRED sub-8x8 PU in a call on s1 and one in a call on s2: the next query counts both, the one after it none"""
    torch = pytest.importorskip("torch")
    ip = [_inter_batch(90 + i, (4, 4), 250, refused=1) for i in range(2)]
    ip_dev = [InterDevice(torch, refs, desc, (4, 4)) for refs, desc, _ in ip]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx = svtav1_hip.Context(0)
    try:
        ip_dev[0].launch(ctx, s1.cuda_stream)
        ip_dev[1].launch(ctx, s2.cuda_stream)
        L, n = svtav1_hip.lib(), C.c_uint32(12345)
        rc = L.svthip_inter_pred_refused(ctx._h, C.byref(n))
        assert rc != 0 and n.value == 2, (rc, n.value, L.svthip_last_error())
        n.value = 12345
        rc = L.svthip_inter_pred_refused(ctx._h, C.byref(n))
        assert rc == 0 and n.value == 0, (rc, n.value)
        assert ctx.inter_pred_refused() == 0
        torch.cuda.synchronize()
        for i, (d, (_, _, w)) in enumerate(zip(ip_dev, ip)):
            d.check(w, f"batch with one refused PU on s{i + 1}")
    finally:
        ctx.close()


# -- host-pointer fused T/Q across calls --------------------------------------------------------------------------------------------

def test_host_tq_across_plane_sizes_and_sample_widths(oracle):
    """svthip_encode_tu_batch on one context: 64x64 TUs on a large plane -> 4x4 on a small plane -> 16-bit planes -> in place (recon ==
    pred); slots 12-15 are laid out from each call's plane size and pool sizes"""
    rng = np.random.default_rng(123)
    steps = [("64x64 on 1024x512", random_encode_batch(rng, 30, 64, 64, pic_w=1024, pic_h=512), False),
             ("4x4 on 64x32", random_encode_batch(rng, 100, 4, 4, pic_w=64, pic_h=32), False),
             ("16x16 on 16-bit 256x128", random_encode_batch(rng, 50, 16, 16, pic_w=256, pic_h=128, bit_depth=10), False),
             ("8x8 in place on 128x64", random_encode_batch(rng, 60, 8, 8, pic_w=128, pic_h=64), True),
             ("64x64 10-bit in place on 1024x512", random_encode_batch(rng, 20, 64, 64, pic_w=1024, pic_h=512, bit_depth=10), True)]
    ctx = svtav1_hip.Context(0)
    try:
        for step, b, in_place in steps:
            want = oracle_encode_batch(oracle, b)
            pred = b["pred"].copy()
            recon = pred if in_place else b["pred"].copy()
            got = ctx.encode_tu_batch(b["src"], pred, recon, b["desc"], b["w"], b["h"], b["qparams"], b["iscan"], len(b["desc"]) * b["n"])
            got["recon"] = recon
            for k in ("recon", "coeff", "qcoeff", "dqcoeff", "eob", "energy", "dist"):
                assert np.array_equal(got[k], want[k]), f"{step}: {k} differs from the oracle"
            if not in_place:
                assert np.array_equal(pred, b["pred"]), f"{step}: the prediction plane was written"
            assert (want["eob"] > 0).any()
    finally:
        ctx.close()


# -- two contexts interleaved -------------------------------------------------------------------------------------------------------

def test_two_contexts_interleaved(expected):
    """context X at A and context Y at B, alternating, each reserving 4K in between: each matches the oracle at every step"""
    X, Y = svtav1_hip.Context(0), svtav1_hip.Context(0)
    try:
        rx, ry = HostMe(X, expected, True, 85), HostMe(Y, expected, True, 85)
        rx.me(A, "X at A")
        ry.me(B, "Y at B")
        X.reserve(BIG[0], BIG[1], 85, 1, host_forms=True)
        ry.me(B, "Y at B after X reserved")
        rx.me(A, "X at A after its reserve")
        Y.reserve(BIG[0], BIG[1], 209, 1, host_forms=True)
        rx.me(A, "X at A after Y reserved")
        ry.me(B, "Y at B after its reserve")
    finally:
        X.close()
        Y.close()
