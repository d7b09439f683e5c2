"""GPU: mode decision's interpolation-filter search (svthip_md_model_rd_batch_dev, svthip_md_interp_filter_search_batch_dev) through the C
ABI, bit-exact against the reference's fixture (tests/golden/md_ifs.npz) and the restatement (tests/md_ifs_util.py).  The model entry runs
with every plane inside a larger buffer of garbage, once with a stride and a base that are multiples of 4 and once each 1, 2 and 3 bytes
into its buffer at an odd stride; the samples right around every tile are 0 and 255, so a sum that strays changes.  The search entry runs
the fixture's candidates in its three modes, writes the chosen filters back into the PU descriptors and hands those to
svthip_av1_inter_pred_batch_dev on the same stream."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import inter_pred_util as ipu  # noqa: E402
import md_ifs_util as mu  # noqa: E402
import svtav1_hip  # noqa: E402
from test_md_fast_gpu import LAYOUTS, _dev, _Planes  # noqa: E402  (planes inside garbage at the four layouts)

pytestmark = pytest.mark.gpu

BAD = "80001005"
N_FIXTURE = 32


def _run_model(torch, ctx, src, pool, desc, w, h, quantizer, stream=None):
    d_desc = _dev(torch, desc)
    d_result = torch.full((len(desc) * 32 + 32,), 0x77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.md_model_rd_batch_dev(src.arg, pool.arg, d_desc.data_ptr(), len(desc), w, h, quantizer, d_result.data_ptr(), stream=stream)
    ctx.synchronize()
    if stream is not None:
        torch.cuda.synchronize()
    raw = d_result.cpu().numpy()
    assert (raw[len(desc) * 32:] == 0x77).all(), "wrote behind the last result"
    return raw[:len(desc) * 32].view(mu.MODEL_RESULT_DTYPE)


@pytest.mark.parametrize("z", range(len(mu.SIZES)))
def test_model_rd_every_size_bit_exact(hip_ctx, z):
    torch = pytest.importorskip("torch")
    w, h = mu.SIZES[z]
    src, pool = mu.model_planes(z)
    fx = mu.fixture()
    mid = mu.QUANTIZERS[2]
    batches = {n: mu.model_descriptors(z, n, variant=n) for n in (1, 5, 67)}
    batches[13] = mu.model_descriptors(z, 13)
    want = {n: mu.model_rd(src, pool, d, w, h, mid)[0] for n, d in batches.items()}
    hip_ctx.inter_pred_refused()
    for shift in LAYOUTS:
        d_src, d_pool = _Planes(torch, src, shift), _Planes(torch, pool, shift)
        for k, quantizer in enumerate(mu.QUANTIZERS):   # the reference's rows, every quantizer
            if shift == 0 or quantizer == mid:
                got = _run_model(torch, hip_ctx, d_src, d_pool, batches[13], w, h, quantizer)
                ref = np.ascontiguousarray(fx[f"model_z{z}_q{k}"]).view(mu.MODEL_RESULT_DTYPE).reshape(-1)
                bad = np.flatnonzero(got != ref)
                assert bad.size == 0, ((w, h), shift, quantizer, bad[:6], got[bad[:3]], ref[bad[:3]])
        assert np.array_equal(want[13], np.ascontiguousarray(fx[f"model_z{z}_q2"]).view(mu.MODEL_RESULT_DTYPE).reshape(-1)), "the restatement left the fixture"
        for n in ((1, 5, 67) if shift in (0, 3) else (5,)):
            got = _run_model(torch, hip_ctx, d_src, d_pool, batches[n], w, h, mid)
            bad = np.flatnonzero(got != want[n])
            assert bad.size == 0, ((w, h), shift, n, bad[:6], got[bad[:3]], want[n][bad[:3]])
    hip_ctx.md_model_rd_batch_dev(None, None, None, 0, w, h, mid, None)   # n_tiles == 0: nothing is looked at
    assert hip_ctx.inter_pred_refused() == 0


def test_model_rd_largest_sums(hip_ctx):
    """one 128 x 128 tile in which every difference is 255, the largest quantizer, a 32-bit lambda and a rate near INT32_MAX"""
    torch = pytest.importorskip("torch")
    src, pred, desc = mu.extreme_tile()
    got = _run_model(torch, hip_ctx, _Planes(torch, src, 0), _Planes(torch, pred, 1), desc, 128, 128, mu.QUANTIZERS[-1])
    ref = np.ascontiguousarray(mu.fixture()["model_extreme"]).view(mu.MODEL_RESULT_DTYPE).reshape(-1)
    assert got[0]["sse"].tolist() == [128 * 128 * 255 * 255, 64 * 64 * 255 * 255, 64 * 64 * 255 * 255]
    assert np.array_equal(got, ref) and np.array_equal(got, mu.model_rd(src, pred, desc, 128, 128, mu.QUANTIZERS[-1])[0])


# ------------------------------------------------------------------------------------------------ the search

class _Search:
    """the pictures of md_ifs_util.search_pictures on the device"""

    def __init__(self, torch):
        self.ref0, self.ref1, src = mu.search_pictures()
        self.src = ipu.Picture(*src, 0)
        self.dev = [ipu.to_device(p) for p in (self.ref0, self.ref1, self.src)]
        self.planes = [ipu.planes_of(d, p) for d, p in zip(self.dev, (self.ref0, self.ref1, self.src))]


@pytest.fixture(scope="module")
def pictures():
    torch = pytest.importorskip("torch")
    return _Search(torch)


def _tile_grid(pu, w, h):
    """dst_origin of every candidate for the prediction that follows the search: a grid of tiles, 16 across; returns the blank picture"""
    n = len(pu)
    pu["dst_origin_x"], pu["dst_origin_y"] = (np.arange(n) % 16) * w, (np.arange(n) // 16) * h
    pw, ph = 16 * w, ((n + 15) // 16) * h
    return ipu.Picture(np.full((ph, pw), 0x55, np.uint8), np.full((ph // 2, pw // 2), 0x55, np.uint8), np.full((ph // 2, pw // 2), 0x55, np.uint8), 0)


def _run_search(torch, ctx, P, pu, f, w, h, search_mode, dual, quantizer, write_back=1, stream=None, predict=True):
    """the search, then -- on the same stream, nothing in between -- the prediction from the descriptors it patched.  Returns
    (IFS_RESULT_DTYPE[n], the descriptors read back, the predicted picture or None)"""
    pu = pu.copy()
    blank = _tile_grid(pu, w, h)
    d_pu, d_f = _dev(torch, pu), _dev(torch, f)
    d_result = torch.full((len(pu) * 32 + 32,), 0x77, dtype=torch.uint8, device="cuda:0")
    d_dst = ipu.to_device(blank)
    torch.cuda.synchronize()
    ctx.md_interp_filter_search_batch_dev(P.planes[0], P.planes[1], P.planes[2], d_pu.data_ptr(), d_f.data_ptr(), len(pu), w, h, search_mode, dual, quantizer,
                                          write_back, d_result.data_ptr(), stream=stream)
    if predict:
        ctx.av1_inter_pred_batch_dev(P.planes[0], P.planes[1], ipu.planes_of(d_dst, blank), d_pu.data_ptr(), len(pu), w, h, stream=stream)
    ctx.synchronize()
    torch.cuda.synchronize()
    raw = d_result.cpu().numpy()
    assert (raw[len(pu) * 32:] == 0x77).all(), "wrote behind the last result"
    after = d_pu.cpu().numpy().view(svtav1_hip.INTER_PU_DESC_DTYPE)
    changed = [k for k in after.dtype.names if k != "interp_filters" and not np.array_equal(after[k], pu[k])]
    assert not changed, ("the search changed descriptor fields other than interp_filters", changed)
    pic = ipu.Picture(d_dst["y"].cpu().numpy(), d_dst["cb"].cpu().numpy(), d_dst["cr"].cpu().numpy(), 0) if predict else None
    return raw[:len(pu) * 32].view(mu.IFS_RESULT_DTYPE), after, pic


def _check_tiles(pic, after, got, trials, w, h):
    """every tile of the prediction that followed is the restatement's prediction with the chosen filters"""
    for k, (d, r) in enumerate(zip(after, got)):
        assert int(d["interp_filters"]) == int(r["interp_filters"]), k
        x, y = int(d["dst_origin_x"]), int(d["dst_origin_y"])
        t = trials[k].tile(int(r["best_trial"]))
        assert np.array_equal(pic.y[y:y + h, x:x + w], t.y), ("luma", k)
        assert np.array_equal(pic.cb[y // 2:(y + h) // 2, x // 2:(x + w) // 2], t.cb) and np.array_equal(pic.cr[y // 2:(y + h) // 2, x // 2:(x + w) // 2], t.cr), ("chroma", k)


@pytest.mark.parametrize("size", mu.SEARCH_SIZES)
def test_search_matches_reference_fixture(hip_ctx, pictures, size):
    torch = pytest.importorskip("torch")
    w, h = size
    quantizer = mu.search_quantizer(size)
    pu, f, trials = mu.search_trials(size, N_FIXTURE, quantizer)
    hip_ctx.inter_pred_refused()
    for name, search_mode, dual in mu.MODES:
        ref = np.ascontiguousarray(mu.fixture()[f"search_{w}x{h}_{name}"]).view(mu.IFS_RESULT_DTYPE).reshape(-1)
        got, after, pic = _run_search(torch, hip_ctx, pictures, pu, f, w, h, search_mode, dual, quantizer)
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (size, name, bad[:6], got[bad[:3]], ref[bad[:3]])
        want, refused = mu.search(trials, search_mode, dual)
        assert refused == 0 and np.array_equal(got, want), (size, name)
        _check_tiles(pic, after, got, trials, w, h)
    # without write_back the descriptors keep the filters they came with
    got, after, _ = _run_search(torch, hip_ctx, pictures, pu, f, w, h, 1, 1, quantizer, write_back=0, predict=False)
    assert np.array_equal(after["interp_filters"], pu["interp_filters"]) and np.array_equal(got, mu.search(trials, 1, 1)[0])
    assert hip_ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("n", [1, 7, 150])
def test_search_batches(hip_ctx, pictures, n):
    """1, 7 and 150 candidates: more than one workgroup of walkers and of expanders, the last partial"""
    torch = pytest.importorskip("torch")
    hip_ctx.inter_pred_refused()
    for size in ((8, 8), (16, 8)):
        w, h = size
        quantizer = mu.search_quantizer(size)
        pu, f, trials = mu.search_trials(size, n, quantizer, variant=n)
        for name, search_mode, dual in mu.MODES[:2]:
            got, after, pic = _run_search(torch, hip_ctx, pictures, pu, f, w, h, search_mode, dual, quantizer)
            want, refused = mu.search(trials, search_mode, dual)
            bad = np.flatnonzero(got != want)
            assert refused == 0 and bad.size == 0, (size, name, n, bad[:6], got[bad[:3]], want[bad[:3]])
            _check_tiles(pic, after, got, trials, w, h)
    assert hip_ctx.inter_pred_refused() == 0


def test_search_context_reuse_and_growth(pictures):
    """a second call on the same context with another size and another stream: the scratch grows behind the first call, then is reused"""
    torch = pytest.importorskip("torch")
    ctx = svtav1_hip.Context(0)
    try:
        s = torch.cuda.Stream()
        for size, n, stream, mode in (((8, 8), 7, None, 1), ((64, 64), 20, s.cuda_stream, 2), ((8, 8), 7, None, 1), ((32, 32), 9, s.cuda_stream, 1)):
            w, h = size
            quantizer = mu.search_quantizer(size)
            pu, f, trials = mu.search_trials(size, n, quantizer)
            got, after, pic = _run_search(torch, ctx, pictures, pu, f, w, h, mode, 1, quantizer, stream=stream)
            assert np.array_equal(got, mu.search(trials, mode, 1)[0]), (size, n)
            _check_tiles(pic, after, got, trials, w, h)
        assert ctx.inter_pred_refused() == 0
    finally:
        ctx.close()


def test_device_side_refusals(hip_ctx, pictures):
    """an odd source position, a PU the prediction refuses (edges that put the clamped block far above the padded picture), and in the
    model entry a tile at an odd position: zeroed rows, counted once each, reported once through svthip_inter_pred_refused"""
    torch = pytest.importorskip("torch")
    w, h = 16, 8
    quantizer = mu.search_quantizer((w, h))
    pu, f, trials = mu.search_trials((w, h), 12, quantizer)
    f[3]["src_x"] += 1
    f[8]["src_y"] += 1
    pu[5]["mb_to_bottom_edge"] = -8 * 40000
    pu[10]["mb_to_right_edge"], pu[10]["pred_direction"] = -8 * 200000, 2
    refused = {3, 5, 8, 10}
    hip_ctx.inter_pred_refused()
    for name, search_mode, dual in mu.MODES:
        got, after, _ = _run_search(torch, hip_ctx, pictures, pu, f, w, h, search_mode, dual, quantizer, predict=False)
        want, n_refused = mu.search(trials, search_mode, dual, refused=refused)
        assert n_refused == 4 and np.array_equal(got, want), name
        for k in refused:
            assert got[k].tobytes() == mu.refused_row().tobytes() and int(after[k]["interp_filters"]) == 0
        with pytest.raises(svtav1_hip.SvtHipError, match=rf"{BAD}: 4 PU\(s\) or unit\(s\) refused.*svthip_md_interp_filter_search_batch_dev"):
            hip_ctx.inter_pred_refused()
        assert hip_ctx.inter_pred_refused() == 0

    z = mu.SIZES.index((16, 8))
    src, pool = mu.model_planes(z)
    desc = mu.model_descriptors(z, 9)
    for i, k in ((1, "src_x"), (2, "src_y"), (4, "pred_x"), (7, "pred_y")):
        desc[i][k] += 1
    got = _run_model(torch, hip_ctx, _Planes(torch, src, 0), _Planes(torch, pool, 0), desc, 16, 8, 260)
    want, n_refused = mu.model_rd(src, pool, desc, 16, 8, 260)
    assert n_refused == 4 and np.array_equal(got, want) and all(got[i].tobytes() == bytes(32) for i in (1, 2, 4, 7))
    with pytest.raises(svtav1_hip.SvtHipError, match=rf"{BAD}: 4 PU\(s\) or unit\(s\) refused.*svthip_md_model_rd_batch_dev"):
        hip_ctx.inter_pred_refused()
    assert hip_ctx.inter_pred_refused() == 0


def test_host_side_refusals(pictures):
    torch = pytest.importorskip("torch")
    ctx = svtav1_hip.Context(0)
    try:
        w, h = 8, 8
        pu, f, _ = mu.search_trials((w, h), 4, 260)
        d_pu, d_f = _dev(torch, np.concatenate([pu, pu])), _dev(torch, np.concatenate([f, f]))
        d_result = torch.zeros(6 * 32, dtype=torch.uint8, device="cuda:0")
        z = mu.SIZES.index((w, h))
        src, pool = mu.model_planes(z)
        m_src, m_pool = _Planes(torch, src, 0), _Planes(torch, pool, 0)
        d_m = _dev(torch, mu.model_descriptors(z, 6))
        torch.cuda.synchronize()
        P = pictures.planes
        ok_search = dict(ref0=P[0], ref1=P[1], src=P[2], d_pu_desc=d_pu.data_ptr(), d_ifs_desc=d_f.data_ptr(), n_cand=4, bwidth=w, bheight=h, search_mode=1,
                         enable_dual_filter=1, quantizer=260, write_back=0, d_result=d_result.data_ptr())
        ok_model = dict(src=m_src.arg, pred=m_pool.arg, d_desc=d_m.data_ptr(), n_tiles=4, bwidth=w, bheight=h, quantizer=260, d_result=d_result.data_ptr())
        search, model = ctx.md_interp_filter_search_batch_dev, ctx.md_model_rd_batch_dev

        def refused(words, call, **change):
            with pytest.raises(svtav1_hip.SvtHipError, match=f"{BAD}.*{words}"):
                call(**{**(ok_search if call == search else ok_model), **change})

        def without(planes, plane):
            p = svtav1_hip.InterPlanes()
            for k in ("y", "cb", "cr", "y_stride", "c_stride"):
                setattr(p, k, getattr(planes, k))
            setattr(p, plane, None)
            return p

        for call in (search, model):
            for bw, bh in ((4, 4), (4, 8), (8, 4), (4, 16), (16, 4), (12, 8), (0, 0), (256, 128), (128, 32), (8, 64)):   # the 4-wide and 4-high AV1 sizes too
                refused("not one of the 17 AV1 block sizes with both sides above 4", call, bwidth=bw, bheight=bh)
            refused("not one of the 17", call, bwidth=4, bheight=8, **{"n_cand" if call == search else "n_tiles": 0})   # the size is checked before the count
        for mode in (0, 3, -1):
            refused("search_mode must be 1 .fast. or 2 .full.", search, search_mode=mode)
        refused("search_mode", search, search_mode=0, n_cand=0)
        for call in (search, model):
            for q in (32768, -32769, 1 << 20):
                refused("is not an int16_t value", call, quantizer=q)
        for k in ("ref0", "ref1", "src", "d_pu_desc", "d_ifs_desc", "d_result"):
            refused("null pointer", search, **{k: None})
        for k in ("src", "pred", "d_desc", "d_result"):
            refused("null pointer", model, **{k: None})
        for plane in ("y", "cb", "cr"):
            for k in ("ref0", "ref1", "src"):
                refused("null plane pointer", search, **{k: without(ok_search[k], plane)})
            for k in ("src", "pred"):
                refused("null plane pointer", model, **{k: without(ok_model[k], plane)})
        refused("descriptor array must be 16-byte aligned", search, d_pu_desc=d_pu.data_ptr() + 8)
        refused("must be 16-byte aligned", search, d_ifs_desc=d_f.data_ptr() + 8)
        refused("must be 16-byte aligned", search, d_result=d_result.data_ptr() + 8)
        refused("descriptor array must be 16-byte aligned", model, d_desc=d_m.data_ptr() + 8)
        refused("result array must be 16-byte aligned", model, d_result=d_result.data_ptr() + 8)
        search(None, None, None, None, None, 0, w, h, 2, 0, 260, 1, None)   # n_cand == 0 returns OK
        model(None, None, None, 0, w, h, 260, None)
        search(**ok_search)
        model(**ok_model)
        ctx.synchronize()
        assert ctx.inter_pred_refused() == 0
    finally:
        ctx.close()
