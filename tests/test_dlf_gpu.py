"""GPU: the deblocking entries bit-exact against the reference's fixture (tests/golden/dlf.npz) and the numpy restatement
(tests/dlf_util.py): svthip_av1_[highbd_]loop_filter_frame_dev on every recorded run, inside a larger allocation whose guard must stay
untouched; svthip_av1_[highbd_]loop_filter_sse_table_dev, all 64 entries per search, the reconstruction unchanged, and four levels of a
fresh picture; svthip_lf_level_walk_dev on the reference's and on constructed tables; svthip_av1_[highbd_]pick_filter_level_dev against
the reference's av1_pick_filter_level, its device-side levels then feeding the frame filter; every refusal."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import dlf_util as du  # noqa: E402
import svtav1_hip  # noqa: E402
from test_dlf_vs_ref import fixture, fixture_cases, fixture_picks  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 9   # samples of guard around every plane, odd so that the planes start unaligned to a dword row
FILL = {8: 0xA5, 10: 0x2A5}


class DevPicture:
    """the planes of a picture embedded in larger allocations filled with a guard pattern"""

    def __init__(self, torch, recon, source, bd):
        self.torch, self.bd = torch, bd
        self.host, self.dev, self.keep = [], [], []
        h, w = recon[0].shape
        ptr, stride, sptr, sstride = [], [], [], []
        for p in range(3):
            ph, pw = recon[p].shape
            big = np.full((ph + 2 * GUARD, pw + 2 * GUARD + p), FILL[bd] + p, recon[p].dtype)
            big[GUARD:GUARD + ph, GUARD:GUARD + pw] = recon[p]
            d = torch.from_numpy(big.view(np.uint8).reshape(-1).copy()).to("cuda:0")
            self.host.append(big)
            self.dev.append(d)
            ptr.append(d.data_ptr() + (GUARD * big.shape[1] + GUARD) * big.itemsize)
            stride.append(big.shape[1])
            s = torch.from_numpy(np.ascontiguousarray(source[p]).view(np.uint8).reshape(-1).copy()).to("cuda:0") if source is not None else None
            self.keep.append(s)
            sptr.append(s.data_ptr() if s is not None else None)
            sstride.append(pw if s is not None else 0)
        self.pic = svtav1_hip.make_lf_picture(w, h, ptr, stride, sptr, sstride)

    def planes(self):
        """(planes, guard untouched)"""
        out, ok = [], True
        for p in range(3):
            big = self.dev[p].cpu().numpy().view(self.host[p].dtype).reshape(self.host[p].shape)
            ph, pw = big.shape[0] - 2 * GUARD, big.shape[1] - 2 * GUARD - p
            out.append(big[GUARD:GUARD + ph, GUARD:GUARD + pw].copy())
            mask = np.ones(big.shape, bool)
            mask[GUARD:GUARD + ph, GUARD:GUARD + pw] = False
            ok &= bool(np.all(big[mask] == FILL[self.bd] + p))
        return out, ok


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


@pytest.mark.parametrize("c", range(6))
def test_frame_filter_matches_fixture(hip_ctx, c):
    torch = pytest.importorskip("torch")
    (_, w, h, bd, mi, recon, _, runs, outs) = fixture_cases()[c]
    d_mi = _dev(torch, mi)
    for r, (l0, l1, lu, lv, sharpness, ps, pe) in enumerate(runs):
        P = DevPicture(torch, recon, None, bd)
        d_levels = _dev(torch, np.array([l0, l1, lu, lv], np.int32))
        hip_ctx.av1_loop_filter_frame_dev(P.pic, d_mi.data_ptr(), mi.shape[1], d_levels.data_ptr(), sharpness, ps, pe, bit_depth=bd)
        hip_ctx.synchronize()
        got, guard_ok = P.planes()
        for p in range(3):
            assert np.array_equal(got[p], outs[r][p]), (c, r, p)
        assert guard_ok, (c, r)


@pytest.mark.parametrize("c", range(6))
def test_sse_tables_match_fixture(hip_ctx, c):
    torch = pytest.importorskip("torch")
    (_, w, h, bd, mi, recon, source, _, _) = fixture_cases()[c]
    z = fixture()
    d_mi = _dev(torch, mi)
    P = DevPicture(torch, recon, source, bd)
    for i, (plane, direction, _, _) in enumerate(du.PICK_RUNS):
        d_levels = _dev(torch, z[f"c{c}_table_levels"][i].astype(np.int32))
        d_sse = torch.full((64,), -1, dtype=torch.int64, device="cuda:0")
        hip_ctx.av1_loop_filter_sse_table_dev(P.pic, d_mi.data_ptr(), mi.shape[1], plane, direction, d_levels.data_ptr(), 0, d_sse.data_ptr(),
                                              bit_depth=bd)
        hip_ctx.synchronize()
        assert np.array_equal(d_sse.cpu().numpy().view(np.uint64), z[f"c{c}_table"][i]), (c, plane, direction)
    got, guard_ok = P.planes()
    assert guard_ok and all(np.array_equal(g, r) for g, r in zip(got, recon)), "the table entry changed the reconstruction"


@pytest.mark.parametrize("bd", [8, 10])
def test_sse_levels_of_a_fresh_picture(hip_ctx, bd):
    """136x72 (partial last tile both ways), non-zero sharpness, every (plane, dir): four levels against the restatement"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(500 + bd)
    mi = du.random_mi_grid(rng, 136, 72)
    recon, source = du.random_picture(rng, 136, 72, bd, mi)
    d_mi = _dev(torch, mi)
    P = DevPicture(torch, recon, source, bd)
    levels = (26, 7, 0, 0)
    d_levels = _dev(torch, np.array(levels, np.int32))
    for (plane, direction) in ((0, 2), (0, 0), (0, 1), (1, 0), (2, 0)):
        d_sse = torch.zeros(64, dtype=torch.int64, device="cuda:0")
        hip_ctx.av1_loop_filter_sse_table_dev(P.pic, d_mi.data_ptr(), mi.shape[1], plane, direction, d_levels.data_ptr(), 2, d_sse.data_ptr(),
                                              bit_depth=bd)
        hip_ctx.synchronize()
        got = d_sse.cpu().numpy()
        want = du.sse_table(recon, source, mi, plane, direction, levels, 2, bd, only=(0, 1, 17, 63))
        assert {k: int(got[k]) for k in want} == want, (bd, plane, direction)


def test_walk_matches_fixture(hip_ctx):
    torch = pytest.importorskip("torch")
    z = fixture()
    n = len(z["walk_table"])
    d_tables = _dev(torch, z["walk_table"])
    d_level = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    d_mask = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    for i, (start, only) in enumerate(z["walk_arg"]):
        hip_ctx.lf_level_walk_dev(d_tables.data_ptr() + i * 512, int(start), int(only), d_level.data_ptr() + 4 * i, d_mask.data_ptr() + 8 * i)
    hip_ctx.synchronize()
    assert np.array_equal(d_level.cpu().numpy().astype(np.uint64), z["walk_out"][:, 0])
    assert np.array_equal(d_mask.cpu().numpy().view(np.uint64), z["walk_out"][:, 1])
    assert z["walk_synthetic"].any() and not z["walk_synthetic"].all()


@pytest.mark.parametrize("c", range(6))
def test_pick_matches_reference_and_feeds_the_filter(hip_ctx, c):
    torch = pytest.importorskip("torch")
    (_, w, h, bd, mi, recon, source, _, _) = fixture_cases()[c]
    d_mi = _dev(torch, mi)
    for (last, only, want, _, masks) in fixture_picks(c):
        P = DevPicture(torch, recon, source, bd)
        d_levels = torch.full((4,), -1, dtype=torch.int32, device="cuda:0")
        d_tables = torch.zeros(5 * 64, dtype=torch.int64, device="cuda:0")
        d_masks = torch.zeros(5, dtype=torch.int64, device="cuda:0")
        hip_ctx.av1_pick_filter_level_dev(P.pic, d_mi.data_ptr(), mi.shape[1], last, 0, only, d_levels.data_ptr(), d_tables.data_ptr(),
                                          d_masks.data_ptr(), bit_depth=bd)
        # the levels stay on the device: the frame filter takes the same array
        hip_ctx.av1_loop_filter_frame_dev(P.pic, d_mi.data_ptr(), mi.shape[1], d_levels.data_ptr(), 0, 0, 3, bit_depth=bd)
        hip_ctx.synchronize()
        assert d_levels.cpu().numpy().tolist() == want, (c, last, only)
        assert np.array_equal(d_masks.cpu().numpy().view(np.uint64), masks), (c, last, only)
        filtered = [p.copy() for p in recon]
        du.loop_filter_frame(filtered, mi, want, 0, 0, 3, bd)
        got, guard_ok = P.planes()
        assert guard_ok and all(np.array_equal(g, f) for g, f in zip(got, filtered)), (c, last, only)


def test_pick_filtered_picture_is_the_references(hip_ctx):
    """run 0 of the fixture is the reference's av1_loop_filter_frame; the same levels handed over as a device array that a walk wrote"""
    torch = pytest.importorskip("torch")
    (_, w, h, bd, mi, recon, _, runs, outs) = fixture_cases()[1]
    l0, l1, lu, lv, sharpness, ps, pe = runs[0]
    d_levels = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    for k, level in enumerate((l0, l1, lu, lv)):   # a table whose minimum is the level wanted, walked on the device into slot k
        table = (np.abs(np.arange(64) - level).astype(np.uint64) << np.uint64(20)) + np.uint64(1 << 30)
        d_t = _dev(torch, table)
        hip_ctx.lf_level_walk_dev(d_t.data_ptr(), level, 0, d_levels.data_ptr() + 4 * k)
    P = DevPicture(torch, recon, None, bd)
    hip_ctx.av1_loop_filter_frame_dev(P.pic, _dev(torch, mi).data_ptr(), mi.shape[1], d_levels.data_ptr(), sharpness, ps, pe, bit_depth=bd)
    hip_ctx.synchronize()
    assert d_levels.cpu().numpy().tolist() == [l0, l1, lu, lv]
    got, guard_ok = P.planes()
    assert guard_ok and all(np.array_equal(g, o) for g, o in zip(got, outs[0]))


def test_only_the_planes_of_the_call_are_needed(hip_ctx):
    """a luma-only filtering and a luma table with null chroma entries in the picture; a chroma table with a null luma entry"""
    torch = pytest.importorskip("torch")
    (_, w, h, bd, mi, recon, source, runs, outs) = fixture_cases()[1]
    z = fixture()
    l0, l1, lu, lv, sharpness, _, _ = runs[0]
    d_mi = _dev(torch, mi)
    P = DevPicture(torch, recon, source, bd)
    d_levels = _dev(torch, np.array([l0, l1, lu, lv], np.int32))
    luma = svtav1_hip.make_lf_picture(w, h, [P.pic.recon[0], None, None], list(P.pic.recon_stride), [P.pic.source[0], None, None],
                                      list(P.pic.source_stride))
    cb = svtav1_hip.make_lf_picture(w, h, [None, P.pic.recon[1], None], list(P.pic.recon_stride), [None, P.pic.source[1], None],
                                    list(P.pic.source_stride))
    for pic, i in ((luma, 0), (cb, 3)):
        plane, direction, _, _ = du.PICK_RUNS[i]
        d_at = _dev(torch, z["c1_table_levels"][i].astype(np.int32))
        d_sse = torch.zeros(64, dtype=torch.int64, device="cuda:0")
        hip_ctx.av1_loop_filter_sse_table_dev(pic, d_mi.data_ptr(), mi.shape[1], plane, direction, d_at.data_ptr(), 0, d_sse.data_ptr(), bit_depth=bd)
        hip_ctx.synchronize()
        assert np.array_equal(d_sse.cpu().numpy().view(np.uint64), z["c1_table"][i])
    hip_ctx.av1_loop_filter_frame_dev(luma, d_mi.data_ptr(), mi.shape[1], d_levels.data_ptr(), sharpness, 0, 1, bit_depth=bd)
    hip_ctx.synchronize()
    got, guard_ok = P.planes()
    assert guard_ok and np.array_equal(got[0], outs[0][0]) and np.array_equal(got[1], recon[1]) and np.array_equal(got[2], recon[2])
    with pytest.raises(svtav1_hip.SvtHipError):
        hip_ctx.av1_loop_filter_frame_dev(luma, d_mi.data_ptr(), mi.shape[1], d_levels.data_ptr(), sharpness, 0, 2, bit_depth=bd)


def test_refusals(hip_ctx):
    """refused on the host, before any launch: nothing is written"""
    torch = pytest.importorskip("torch")
    (_, w, h, bd, mi, recon, source, _, _) = fixture_cases()[0]
    d_mi = _dev(torch, mi)
    P = DevPicture(torch, recon, source, bd)
    d_levels = _dev(torch, np.array([20, 20, 20, 20], np.int32))
    d_sse = torch.full((5 * 64,), -1, dtype=torch.int64, device="cuda:0")
    narrow = svtav1_hip.make_lf_picture(w - 4, h, list(P.pic.recon), list(P.pic.recon_stride), list(P.pic.source), list(P.pic.source_stride))
    frame = lambda pic, mi_ptr, *a: hip_ctx.av1_loop_filter_frame_dev(pic, mi_ptr, mi.shape[1], d_levels.data_ptr(), *a)  # noqa: E731
    table = lambda pic, mi_ptr, plane, direction: hip_ctx.av1_loop_filter_sse_table_dev(  # noqa: E731
        pic, mi_ptr, mi.shape[1], plane, direction, d_levels.data_ptr(), 0, d_sse.data_ptr())
    for call in (lambda: frame(narrow, d_mi.data_ptr(), 0, 0, 3), lambda: frame(P.pic, None, 0, 0, 3), lambda: frame(P.pic, d_mi.data_ptr(), 0, 0, 4),
                 lambda: frame(P.pic, d_mi.data_ptr(), 8, 0, 3), lambda: table(narrow, d_mi.data_ptr(), 0, 0), lambda: table(P.pic, d_mi.data_ptr(), 3, 0),
                 lambda: table(P.pic, d_mi.data_ptr(), 0, 3), lambda: table(P.pic, None, 0, 0),
                 lambda: hip_ctx.av1_pick_filter_level_dev(P.pic, None, mi.shape[1], (0, 0, 0, 0), 0, 0, d_levels.data_ptr(), d_sse.data_ptr()),
                 lambda: hip_ctx.av1_pick_filter_level_dev(P.pic, d_mi.data_ptr(), mi.shape[1], (0, 64, 0, 0), 0, 0, d_levels.data_ptr(), d_sse.data_ptr()),
                 lambda: hip_ctx.av1_loop_filter_frame_dev(P.pic, d_mi.data_ptr(), mi.shape[1], d_levels.data_ptr(), 0, 0, 3, bit_depth=12),
                 lambda: hip_ctx.lf_level_walk_dev(None, 0, 0, d_levels.data_ptr())):
        with pytest.raises(svtav1_hip.SvtHipError):
            call()
    hip_ctx.synchronize()
    got, guard_ok = P.planes()
    assert guard_ok and all(np.array_equal(g, r) for g, r in zip(got, recon))
    assert bool((d_sse == -1).all()) and d_levels.cpu().numpy().view(np.int32).tolist() == [20, 20, 20, 20]
