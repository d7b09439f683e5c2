"""GPU: the five motion-analysis entries (svthip_ma_zz_sad_dev, svthip_ma_ac_energy_dev, svthip_ma_distortion_stats_dev,
svthip_ma_global_motion_dev, svthip_ma_sb_flags_dev) through the C ABI, bit-exact against the reference's fixture (tests/golden/ma_stats.npz)
and the restatement (tests/ma_stats_util.py).  The pool is uploaded with picture interiors only and svthip_pa_derive_planes_dev builds the
borders and the 1/16 planes on the device: the real call sequence.  Every output array is filled with a pattern first, so that a word the
entry does not write shows."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import ma_stats_util as mu  # noqa: E402
import svtav1_hip  # noqa: E402
from svtav1_hip import synth  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = {"uint8": 0xAA, "int32": -1431655766, "int64": -6148914691236517206}
TABLE_OUTPUTS = ("rc_me_distortion", "inter_index", "intra_index", "histograms", "full_sb_count", "global_motion", "flags")


def _filled(torch, shape, dtype):
    return torch.full(shape, FILL[str(dtype).split(".")[-1]], dtype=dtype, device="cuda:0")


def _pool(torch, ctx, lumas, stream=None):
    """pictures of one size -> (device pool with borders and 1/16 planes built on the device, descriptors)"""
    laid_out, descs = svtav1_hip.build_picture_pool([synth.PaPicture(p) for p in lumas])
    h, w = lumas[0].shape
    pool = np.full(laid_out.size + 256, 0xEE, np.uint8)
    for luma, d in zip(lumas, descs):
        pool[d.full_offset:d.full_offset + d.full_stride * (h + 136)].reshape(h + 136, d.full_stride)[68:68 + h, 68:68 + w] = luma
    d_pool = torch.from_numpy(pool).to("cuda:0")
    torch.cuda.synchronize()
    ctx.pa_derive_planes_dev(d_pool.data_ptr(), descs, stream=stream)
    return d_pool, descs


def _params(items, ref_index=None):
    out = []
    for j, item in enumerate(items):
        s = mu.signals_dict(item["signals"])
        out.append(svtav1_hip.make_ma_params(**s, ref_index=j if ref_index is None else ref_index[j]))
    return out


def _zz(torch, ctx, pairs, stream=None):
    """[(cur, prev)] in one launch -> sad, zz_cost, non_moving_index [n][n_sb]"""
    n = len(pairs)
    h, w = pairs[0][0].shape
    d_pool, descs = _pool(torch, ctx, [p for pair in pairs for p in pair], stream)
    d = [_filled(torch, (n, mu.n_sbs(w, h)), t) for t in (torch.int32, torch.uint8, torch.uint8)]
    torch.cuda.synchronize()
    ctx.ma_zz_sad_dev(d_pool.data_ptr(), descs[0::2], descs[1::2], *[t.data_ptr() for t in d], stream=stream)
    ctx.synchronize() if stream is None else torch.cuda.synchronize()
    return d[0].cpu().numpy().view(np.uint32), d[1].cpu().numpy(), d[2].cpu().numpy()


def _energy(torch, ctx, items):
    """energy items in one launch -> energy, mean [n][n_sb][5]"""
    n = len(items)
    h, w = items[0]["luma"].shape
    d_pool, descs = _pool(torch, ctx, [it["luma"] for it in items])
    d_y_mean = torch.from_numpy(np.stack([it["y_mean"] for it in items])).to("cuda:0")
    d = [_filled(torch, (n, mu.n_sbs(w, h), 5), torch.int64) for _ in range(2)]
    params = [svtav1_hip.make_ma_params(slice_is_intra=int(it["intra"])) for it in items]
    torch.cuda.synchronize()
    ctx.ma_ac_energy_dev(d_pool.data_ptr(), descs, params, d_y_mean.data_ptr(), d[0].data_ptr(), d[1].data_ptr())
    ctx.synchronize()
    return [t.cpu().numpy().view(np.uint64) for t in d]


def _me_rows(rng, me, stride):
    """[n_sb][85] rows in a table of `stride` rows per SB; the rows past 85 are noise"""
    if stride == 85:
        return me
    out = np.frombuffer(rng.integers(0, 256, me.shape[0] * stride * 24, dtype=np.uint8).tobytes(), mu.ME_DTYPE).reshape(me.shape[0], stride).copy()
    out[:, :85] = me
    return out


def _tables(torch, ctx, w, h, items, stride=85):
    """table items of one geometry in one launch through the three table entries -> {output: [n] + shape}"""
    n, n_sb = len(items), mu.n_sbs(w, h)
    rng = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")  # noqa: E731
    d_me = dev(np.stack([_me_rows(rng, it["me"], stride) for it in items]))
    d_cand, d_y, d_v = dev(np.stack([it["cand"] for it in items])), dev(np.stack([it["y_mean"] for it in items])), dev(np.stack([it["variance"] for it in items]))
    d_rm, d_rv = dev(np.stack([it["ref_mean"] for it in items])), dev(np.stack([it["ref_var"] for it in items]))   # packed per-SB tables: stride 1
    shapes = {"rc_me_distortion": ((n, n_sb), torch.int32), "inter_index": ((n, n_sb), torch.int32), "intra_index": ((n, n_sb), torch.int32),
              "histograms": ((n, 2, 128), torch.int32), "full_sb_count": ((n,), torch.int32), "global_motion": ((n, 12), torch.int32),
              "flags": ((n, n_sb, 4), torch.uint8)}
    d = {k: _filled(torch, s, t) for k, (s, t) in shapes.items()}
    params = _params(items)
    torch.cuda.synchronize()
    ctx.ma_distortion_stats_dev(d_me.data_ptr(), stride, d_cand.data_ptr(), w, h, params, *[d[k].data_ptr() for k in TABLE_OUTPUTS[:5]])
    ctx.ma_global_motion_dev(d_me.data_ptr(), stride, w, h, params, d["global_motion"].data_ptr())
    ctx.ma_sb_flags_dev(d_y.data_ptr(), d_v.data_ptr(), d_rm.data_ptr(), d_rv.data_ptr(), 1, n, d_me.data_ptr(), stride, d_cand.data_ptr(), w, h, params,
                        d["flags"].data_ptr())
    ctx.synchronize()
    return {k: (t.cpu().numpy().view(np.uint32) if k in TABLE_OUTPUTS[:5] else t.cpu().numpy()) for k, t in d.items()}


def _check_tables(got, items, w, h, where):
    for i, item in enumerate(items):
        mine = mu.all_tables(item, w, h)
        for k in TABLE_OUTPUTS:
            assert np.array_equal(got[k][i], mine[k]), (where, i, k, got[k][i], mine[k])
        assert np.array_equal(got["flags"][i], item["flags"]), (where, i)
        if item["compare_global_motion"]:
            assert np.array_equal(got["global_motion"][i][:6], item["global_motion"]), (where, i)
        else:
            assert got["global_motion"][i][11] == 1


@pytest.mark.parametrize("c", range(len(mu.CASES)))
def test_zz_sad_matches_fixture(hip_ctx, c):
    """every pair of a case in one launch"""
    torch = pytest.importorskip("torch")
    w, h, groups = mu.fixture_cases()[c]
    got = _zz(torch, hip_ctx, [(it["cur"], it["prev"]) for it in groups["zz"]])
    for i, item in enumerate(groups["zz"]):
        for k, g in zip(mu.ZZ_KEYS[2:], got):
            assert np.array_equal(g[i], item[k]), ((w, h), i, k, g[i], item[k])


@pytest.mark.parametrize("c", range(len(mu.CASES)))
def test_ac_energy_matches_fixture(hip_ctx, c):
    """the intra pictures and the one that is not, in one launch"""
    torch = pytest.importorskip("torch")
    w, h, groups = mu.fixture_cases()[c]
    got = _energy(torch, hip_ctx, groups["energy"])
    for i, item in enumerate(groups["energy"]):
        for k, g in zip(mu.ENERGY_KEYS[3:], got):
            assert np.array_equal(g[i], item[k]), ((w, h), i, k, g[i], item[k])


@pytest.mark.parametrize("stride", (85, 209))
@pytest.mark.parametrize("c", range(len(mu.CASES)))
def test_table_entries_match_fixture(hip_ctx, c, stride):
    """every table of a case in one launch, the intra picture among the others; both ME table strides"""
    torch = pytest.importorskip("torch")
    w, h, groups = mu.fixture_cases()[c]
    _check_tables(_tables(torch, hip_ctx, w, h, groups["tables"], stride), groups["tables"], w, h, ((w, h), stride))


def test_batch_of_three_equals_three_single_launches(hip_ctx):
    torch = pytest.importorskip("torch")
    w, h, groups = mu.fixture_cases()[2]      # 200x136
    pairs = [(it["cur"], it["prev"]) for it in groups["zz"][:3]]
    batch = _zz(torch, hip_ctx, pairs)
    for i, pair in enumerate(pairs):
        for b, s in zip(batch, _zz(torch, hip_ctx, [pair])):
            assert np.array_equal(b[i], s[0]), ("zz", i)
    three = [groups["energy"][i] for i in (2, 6, 3)]   # noise, the same picture as a non-intra one, the checkerboard
    batch = _energy(torch, hip_ctx, three)
    for i, item in enumerate(three):
        for b, s in zip(batch, _energy(torch, hip_ctx, [item])):
            assert np.array_equal(b[i], s[0]), ("energy", i)
    three = [groups["tables"][i] for i in (0, 5, 1)]   # pan, intra, tilt
    batch = _tables(torch, hip_ctx, w, h, three)
    for i, item in enumerate(three):
        single = _tables(torch, hip_ctx, w, h, [item])
        for k in TABLE_OUTPUTS:
            assert np.array_equal(batch[k][i], single[k][0]), ("tables", i, k)


def test_intra_pictures_alone_need_no_me_table(hip_ctx):
    """the second arm: every picture intra, d_me and the reference tables NULL"""
    torch = pytest.importorskip("torch")
    w, h, groups = mu.fixture_cases()[2]
    item = groups["tables"][5]
    assert mu.signals_dict(item["signals"])["slice_is_intra"]
    n_sb = mu.n_sbs(w, h)
    d_cand = torch.from_numpy(item["cand"].view(np.int32)).to("cuda:0")
    d_y, d_v = torch.from_numpy(item["y_mean"]).to("cuda:0"), torch.from_numpy(item["variance"].view(np.int16)).to("cuda:0")
    d = [_filled(torch, (n_sb,), torch.int32) for _ in range(3)] + [_filled(torch, (256,), torch.int32), _filled(torch, (1,), torch.int32)]
    d_flags = _filled(torch, (n_sb, 4), torch.uint8)
    params = _params([item])
    hip_ctx.ma_distortion_stats_dev(None, 85, d_cand.data_ptr(), w, h, params, *[t.data_ptr() for t in d])
    hip_ctx.ma_sb_flags_dev(d_y.data_ptr(), d_v.data_ptr(), None, None, 0, 0, None, 85, None, w, h, params, d_flags.data_ptr())
    hip_ctx.synchronize()
    mine = mu.all_tables(item, w, h)
    for k, t in zip(TABLE_OUTPUTS[:5], d):
        assert np.array_equal(t.cpu().numpy().view(np.uint32).reshape(np.shape(mine[k])), mine[k]), k
    assert not d_flags.cpu().numpy().any()


def test_caller_stream_without_synchronisation(hip_ctx):
    torch = pytest.importorskip("torch")
    w, h, groups = mu.fixture_cases()[1]
    item = groups["zz"][0]
    s = torch.cuda.Stream()
    got = _zz(torch, hip_ctx, [(item["cur"], item["prev"])], stream=s.cuda_stream)
    for k, g in zip(mu.ZZ_KEYS[2:], got):
        assert np.array_equal(g[0], item[k]), k


def test_small_large_small_on_one_context(hip_ctx):
    """call-sequence state: 64x64, then 256x256, then 64x64 again through all five entries of one context"""
    torch = pytest.importorskip("torch")
    cases = mu.fixture_cases()
    for c in (0, 3, 0):
        w, h, groups = cases[c]
        zz_items, tables = groups["zz"][:2], groups["tables"][:3]
        got = _zz(torch, hip_ctx, [(it["cur"], it["prev"]) for it in zz_items])
        for i, item in enumerate(zz_items):
            for k, g in zip(mu.ZZ_KEYS[2:], got):
                assert np.array_equal(g[i], item[k]), (c, "zz", i, k)
        got = _energy(torch, hip_ctx, groups["energy"][2:4])
        for i, item in enumerate(groups["energy"][2:4]):
            for k, g in zip(mu.ENERGY_KEYS[3:], got):
                assert np.array_equal(g[i], item[k]), (c, "energy", i, k)
        _check_tables(_tables(torch, hip_ctx, w, h, tables), tables, w, h, c)


def test_refused_arguments(hip_ctx):
    """the library's error with a text, and nothing launched: the outputs keep their fill"""
    torch = pytest.importorskip("torch")
    ctx = hip_ctx
    w, h, groups = mu.fixture_cases()[1]      # 136x72
    zz_item, en_item, tb = groups["zz"][0], groups["energy"][2], groups["tables"][0]
    d_pool, descs = _pool(torch, ctx, [zz_item["cur"], zz_item["prev"]])
    n_sb = mu.n_sbs(w, h)
    out = torch.full((1 << 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
    o = [out.data_ptr() + 4096 * k for k in range(8)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")  # noqa: E731
    d_me, d_cand, d_y, d_v = dev(tb["me"]), dev(tb["cand"]), dev(tb["y_mean"]), dev(tb["variance"])
    d_rm, d_rv = dev(tb["ref_mean"]), dev(tb["ref_var"])
    inter, intra = _params([tb]), [svtav1_hip.make_ma_params(slice_is_intra=1)]

    def changed(d, **kw):
        d = svtav1_hip.PaPictureDesc.from_buffer_copy(d)
        for k, v in kw.items():
            setattr(d, k, v)
        return [d]

    def zz(cur=descs[:1], prev=descs[1:], pool=d_pool.data_ptr(), outs=o[:3]):
        ctx.ma_zz_sad_dev(pool, cur, prev, *outs)

    def energy(pics=descs[:1], params=intra, y=d_y.data_ptr(), outs=o[:2]):
        ctx.ma_ac_energy_dev(d_pool.data_ptr(), pics, params, y, *outs)

    def dist(me=d_me.data_ptr(), stride=85, cand=d_cand.data_ptr(), ww=w, hh=h, params=inter, outs=o[:5]):
        ctx.ma_distortion_stats_dev(me, stride, cand, ww, hh, params, *outs)

    def gmot(me=d_me.data_ptr(), stride=85, ww=w, hh=h, params=inter, out_ptr=o[0]):
        ctx.ma_global_motion_dev(me, stride, ww, hh, params, out_ptr)

    def flags(y=d_y.data_ptr(), rm=d_rm.data_ptr(), rv=d_rv.data_ptr(), rs=1, nref=1, me=d_me.data_ptr(), stride=85, cand=d_cand.data_ptr(), ww=w, params=inter,
              out_ptr=o[0]):
        ctx.ma_sb_flags_dev(y, d_v.data_ptr(), rm, rv, rs, nref, me, stride, cand, ww, h, params, out_ptr)

    refused = [
        # mismatched geometry, planes that are too narrow, NULL pointers, too many pictures
        lambda: zz(prev=changed(descs[1], width=128)), lambda: zz(prev=changed(descs[1], height=64)), lambda: zz(cur=changed(descs[0], width=132)),
        lambda: zz(cur=changed(descs[0], sixteenth_stride=(w >> 2) + 30)), lambda: zz(prev=changed(descs[1], full_stride=descs[1].full_stride - 4)),
        lambda: zz(pool=None), lambda: zz(outs=[o[0], None, o[2]]), lambda: zz(cur=descs[:1] * 33, prev=descs[1:] * 33), lambda: zz(outs=[o[0] + 2, o[1], o[2]]),
        lambda: energy(y=None), lambda: energy(outs=[o[0] + 4, o[1]]), lambda: energy(pics=changed(descs[0], full_stride=w + 134)),
        # the arm that reads a table it was not given
        lambda: dist(me=None), lambda: dist(cand=None), lambda: dist(stride=100), lambda: dist(ww=132), lambda: dist(outs=[o[0], o[1], o[2], None, o[4]]),
        lambda: dist(params=inter * 33),
        # no complete SB: the reference divides by their count
        lambda: gmot(ww=56), lambda: gmot(hh=56), lambda: gmot(me=None), lambda: gmot(stride=84), lambda: gmot(out_ptr=None),
        lambda: gmot(params=[svtav1_hip.make_ma_params(hierarchical_levels=6)]), lambda: gmot(params=[svtav1_hip.make_ma_params(temporal_layer_index=6)]),
        lambda: flags(rm=None), lambda: flags(rv=None), lambda: flags(me=None), lambda: flags(cand=None), lambda: flags(rs=0), lambda: flags(nref=0),
        lambda: flags(y=None), lambda: flags(out_ptr=None), lambda: flags(ww=133)]
    for k, call in enumerate(refused):
        with pytest.raises(svtav1_hip.SvtHipError, match="80001005") as e:
            call()
        assert len(str(e.value)) > 20, k      # the error carries a text
    ctx.synchronize()
    assert (out.cpu().numpy() == 0xAA).all()
    # and the same calls, unchanged, are accepted
    zz(), energy(), dist(), gmot(ww=136, hh=72), flags()
    ctx.synchronize()
    assert not (out.cpu().numpy() == 0xAA).all()
