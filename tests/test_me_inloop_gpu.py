"""In-loop motion estimation on the device against tests/golden/inloop_me.npz (what the reference's in_loop_motion_estimation_sblock leaves
with use_subpel_flag = 0 and 1): every fixture case through each stage entry and through the one-call entry, without and with the refinement, the side-of-4 block set, the centres,
scratch reuse across calls of different size, and one refusal per validator arm.  Every plane is a tensor of exactly its stated size: the
source unpadded, the reference with the 64-sample border the header states."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import me_inloop_util as iu  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def cases():
    return iu.fixture_cases(iu.load_fixture())


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _settled():
    """the context's stream does not wait for the stream the tensors above were filled on: let the fills finish before anything is launched"""
    import torch
    torch.cuda.synchronize()


def _host(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


class Planes:
    """the planes of one (case, list) on the device with their geometry"""

    def __init__(self, src, ref, ctr, border=iu.BORDER):
        h, w = src.shape
        rp = iu.pad_plane(ref, border)
        self.w, self.h, self.n_sb = w, h, len(iu.sb_origins(w, h))
        self.src_geom, self.ref_geom = (w, 0, 0), (rp.shape[1], border, border)
        self.d_src, self.d_ref = _dev(src), _dev(rp)
        self.d_sb = _dev(iu.sb_origins(w, h).astype(np.uint16))
        self.d_center = _dev(np.asarray(ctr, np.int16))


def _outputs(n_sb, fill=0):
    """(best_sad, best_mv, inloop_mv) on the device, the first two filled with `fill`"""
    import torch
    words = np.full(n_sb * iu.N_BLOCKS, fill, np.uint32)
    return _dev(words), _dev(words), torch.zeros(n_sb * iu.N_BLOCKS * 2, dtype=torch.int16, device="cuda:0")


@pytest.mark.parametrize("index", range(6))
def test_stage_entries_and_one_call_entry_equal_the_reference(hip_ctx, cases, index):
    import torch
    name, src, refs, ctr, aw, ah, want = cases[index]
    for l, ref in enumerate(refs):
        p = Planes(src, ref, ctr[l])
        n = p.n_sb
        # stage by stage
        d_desc = torch.zeros(n * 8, dtype=torch.int32, device="cuda:0")
        d_sad, d_mv, d_out = _outputs(n)
        _settled()
        hip_ctx.inloop_area_dev(p.d_center.data_ptr(), p.d_sb.data_ptr(), n, p.w, p.h, p.src_geom, p.ref_geom, aw, ah, d_desc.data_ptr())
        hip_ctx.inloop_fullpel_search_dev(p.d_src.data_ptr(), p.w, p.d_ref.data_ptr(), p.ref_geom[0], d_desc.data_ptr(), n, 0, d_sad.data_ptr(), d_mv.data_ptr())
        hip_ctx.inloop_pack_dev(d_mv.data_ptr(), n, d_out.data_ptr())
        hip_ctx.synchronize()
        assert np.array_equal(_host(d_desc, np.int32, (n, 8)), want["desc"][l]), (name, l, "desc")
        assert np.array_equal(_host(d_sad, np.uint32, (n, iu.N_BLOCKS)), want["best_sad"][l]), (name, l, "best_sad")
        assert np.array_equal(_host(d_mv, np.uint32, (n, iu.N_BLOCKS)), want["best_mv"][l]), (name, l, "best_mv")
        assert np.array_equal(_host(d_out, np.int16, (n, iu.N_BLOCKS, 2)), want["inloop_mv"][l]), (name, l, "inloop_mv")
        # one call
        d_sad, d_mv, d_out = _outputs(n)
        _settled()
        hip_ctx.inloop_search_dev(p.d_src.data_ptr(), p.src_geom, p.d_ref.data_ptr(), p.ref_geom, p.w, p.h, p.d_center.data_ptr(), p.d_sb.data_ptr(), n, aw, ah,
                                  d_sad.data_ptr(), d_mv.data_ptr(), d_out.data_ptr())
        hip_ctx.synchronize()
        assert np.array_equal(_host(d_sad, np.uint32, (n, iu.N_BLOCKS)), want["best_sad"][l]), (name, l, "one call: best_sad")
        assert np.array_equal(_host(d_mv, np.uint32, (n, iu.N_BLOCKS)), want["best_mv"][l]), (name, l, "one call: best_mv")
        assert np.array_equal(_host(d_out, np.int16, (n, iu.N_BLOCKS, 2)), want["inloop_mv"][l]), (name, l, "one call: inloop_mv")


@pytest.mark.parametrize("index", range(6))
def test_subpel_entry_and_one_call_entry_equal_the_reference(hip_ctx, cases, index):
    """the reference plane has exactly the 68-sample border the header states for the refinement"""
    import svtav1_hip
    import torch
    name, src, refs, ctr, aw, ah, want = cases[index]
    sbs = iu.sb_origins(src.shape[1], src.shape[0])
    for l, ref in enumerate(refs):
        p = Planes(src, ref, ctr[l], iu.SUBPEL_BORDER)
        n = p.n_sb
        keep = ~want["sub_stale"][l]
        desc = iu.area(ctr[l], sbs, p.w, p.h, p.src_geom, p.ref_geom, aw, ah)
        # the stage entry on the fixture's full-pel results, all blocks and the side-of-4 set
        for block_set in (svtav1_hip.INLOOP_BLOCKS_ALL, svtav1_hip.INLOOP_BLOCKS_SIDE_4):
            d_desc, d_sad, d_mv = _dev(desc), _dev(want["best_sad"][l]), _dev(want["best_mv"][l])
            _settled()
            hip_ctx.inloop_subpel_search_dev(p.d_src.data_ptr(), p.w, p.d_ref.data_ptr(), p.ref_geom[0], d_desc.data_ptr(), n, block_set, d_sad.data_ptr(), d_mv.data_ptr())
            hip_ctx.synchronize()
            sad, mv = _host(d_sad, np.uint32, (n, iu.N_BLOCKS)), _host(d_mv, np.uint32, (n, iu.N_BLOCKS))
            m = keep & (iu.SIDE_4[None, :] if block_set else True)
            assert np.array_equal(sad[m], want["sub_best_sad"][l][m]) and np.array_equal(mv[m], want["sub_best_mv"][l][m]), (name, l, block_set)
            if block_set:   # the other 209 slots keep what they held
                assert np.array_equal(sad[:, ~iu.SIDE_4], want["best_sad"][l][:, ~iu.SIDE_4]) and np.array_equal(mv[:, ~iu.SIDE_4], want["best_mv"][l][:, ~iu.SIDE_4])
        # one call
        d_sad, d_mv, d_out = _outputs(n)
        _settled()
        hip_ctx.inloop_search_dev(p.d_src.data_ptr(), p.src_geom, p.d_ref.data_ptr(), p.ref_geom, p.w, p.h, p.d_center.data_ptr(), p.d_sb.data_ptr(), n, aw, ah,
                                  d_sad.data_ptr(), d_mv.data_ptr(), d_out.data_ptr(), use_subpel=True)
        hip_ctx.synchronize()
        assert np.array_equal(_host(d_sad, np.uint32, (n, iu.N_BLOCKS))[keep], want["sub_best_sad"][l][keep]), (name, l, "one call: best_sad")
        assert np.array_equal(_host(d_mv, np.uint32, (n, iu.N_BLOCKS))[keep], want["sub_best_mv"][l][keep]), (name, l, "one call: best_mv")
        kc = keep[:, iu.PACK_SOURCE]
        assert np.array_equal(_host(d_out, np.int16, (n, iu.N_BLOCKS, 2))[kc], want["sub_inloop_mv"][l][kc]), (name, l, "one call: inloop_mv")


@pytest.mark.parametrize("index", [0, 1, 5])
def test_side_4_equals_all_on_its_640_blocks_and_leaves_the_rest(hip_ctx, cases, index):
    import svtav1_hip
    name, src, refs, ctr, aw, ah, want = cases[index]
    p = Planes(src, refs[0], ctr[0])
    n = p.n_sb
    d_desc = _dev(want["desc"][0])
    d_sad, d_mv, _ = _outputs(n, SENTINEL)
    _settled()
    hip_ctx.inloop_fullpel_search_dev(p.d_src.data_ptr(), p.w, p.d_ref.data_ptr(), p.ref_geom[0], d_desc.data_ptr(), n, svtav1_hip.INLOOP_BLOCKS_SIDE_4,
                                      d_sad.data_ptr(), d_mv.data_ptr())
    hip_ctx.synchronize()
    sad, mv = _host(d_sad, np.uint32, (n, iu.N_BLOCKS)), _host(d_mv, np.uint32, (n, iu.N_BLOCKS))
    assert np.array_equal(sad[:, iu.SIDE_4], want["best_sad"][0][:, iu.SIDE_4]) and np.array_equal(mv[:, iu.SIDE_4], want["best_mv"][0][:, iu.SIDE_4]), name
    assert (sad[:, ~iu.SIDE_4] == SENTINEL).all() and (mv[:, ~iu.SIDE_4] == SENTINEL).all() and int((~iu.SIDE_4).sum()) == 209, name


def test_area_outside_the_legal_range_is_searched_as_the_nearest_legal_one(hip_ctx, cases):
    """a hand-written descriptor: width 0 is searched and decoded as width 1"""
    name, src, refs, ctr, aw, ah, want = cases[1]
    p = Planes(src, refs[0], ctr[0])
    bad, legal = want["desc"][0].copy(), want["desc"][0].copy()
    bad[:, 4], legal[:, 4] = 0, 1
    rp = iu.pad_plane(refs[0])
    sad, mv = iu.fullpel(src.reshape(-1), p.w, rp.reshape(-1), rp.shape[1], legal)
    d_desc = _dev(bad)
    d_sad, d_mv, _ = _outputs(1)
    _settled()
    hip_ctx.inloop_fullpel_search_dev(p.d_src.data_ptr(), p.w, p.d_ref.data_ptr(), p.ref_geom[0], d_desc.data_ptr(), 1, 0, d_sad.data_ptr(), d_mv.data_ptr())
    hip_ctx.synchronize()
    assert np.array_equal(_host(d_sad, np.uint32, (1, iu.N_BLOCKS)), sad) and np.array_equal(_host(d_mv, np.uint32, (1, iu.N_BLOCKS)), mv)


def test_centres_from_a_result_table(hip_ctx):
    import svtav1_hip
    import torch
    rng = np.random.default_rng(3)
    for stride in (85, 209):
        rows = np.zeros((7, stride), svtav1_hip.ME_CU_RESULT_DTYPE)
        for k in ("xMvL0", "yMvL0", "xMvL1", "yMvL1"):
            rows[k] = rng.integers(-2000, 2000, rows.shape)
        rows["xMvL0"][0, 0], rows["yMvL1"][1, 0] = -1, -7      # arithmetic shift: -1 >> 2 = -1, -7 >> 2 = -2
        d_rows = _dev(rows)
        for l in (0, 1):
            d_c = torch.zeros(14, dtype=torch.int16, device="cuda:0")
            _settled()
            hip_ctx.inloop_centers_dev(d_rows.data_ptr(), stride, l, 7, d_c.data_ptr())
            hip_ctx.synchronize()
            assert np.array_equal(_host(d_c, np.int16, (7, 2)), iu.centers(rows, l)), (stride, l)


def test_two_calls_on_one_context_the_larger_first(cases):
    import svtav1_hip
    ctx = svtav1_hip.Context(0)
    try:
        for index in (0, 1, 0):   # 6 superblocks, then 1, then 6 again: the descriptor scratch is reused, never regrown
            name, src, refs, ctr, aw, ah, want = cases[index]
            p = Planes(src, refs[0], ctr[0])
            d_sad, d_mv, d_out = _outputs(p.n_sb)
            _settled()
            ctx.inloop_search_dev(p.d_src.data_ptr(), p.src_geom, p.d_ref.data_ptr(), p.ref_geom, p.w, p.h, p.d_center.data_ptr(), p.d_sb.data_ptr(), p.n_sb, aw, ah,
                                  d_sad.data_ptr(), d_mv.data_ptr(), d_out.data_ptr())
            ctx.synchronize()
            assert np.array_equal(_host(d_sad, np.uint32, (p.n_sb, iu.N_BLOCKS)), want["best_sad"][0]), name
            assert np.array_equal(_host(d_out, np.int16, (p.n_sb, iu.N_BLOCKS, 2)), want["inloop_mv"][0]), name
        ctx.reserve(1920, 1080, svtav1_hip.INLOOP_ME_PU_COUNT)
    finally:
        ctx.close()


def test_refusals_return_an_error(hip_ctx, cases):
    import svtav1_hip
    name, src, refs, ctr, aw, ah, want = cases[1]
    p = Planes(src, refs[0], ctr[0])
    d_desc = _dev(want["desc"][0])
    d_sad, d_mv, d_out = _outputs(1)
    S, R, C, B = p.d_src.data_ptr(), p.d_ref.data_ptr(), p.d_center.data_ptr(), p.d_sb.data_ptr()
    _settled()

    def search(**kw):
        a = dict(d_src=S, area_w=aw, area_h=ah, use_subpel=False, block_set=0, d_sad=d_sad.data_ptr())
        a.update(kw)
        hip_ctx.inloop_search_dev(a["d_src"], p.src_geom, R, p.ref_geom, p.w, p.h, C, B, 1, a["area_w"], a["area_h"], a["d_sad"], d_mv.data_ptr(), d_out.data_ptr(),
                                  use_subpel=a["use_subpel"], block_set=a["block_set"])

    refusals = [
        ("null", lambda: search(d_src=None)), ("null", lambda: search(d_sad=None)),
        ("1..127", lambda: search(area_w=0)), ("1..127", lambda: search(area_h=128)),
        ("block_set", lambda: search(block_set=2)), ("border of 66", lambda: search(use_subpel=True)),   # these planes have the 64 of the full-pel search
        ("null", lambda: hip_ctx.inloop_subpel_search_dev(S, p.w, R, p.ref_geom[0], d_desc.data_ptr(), 1, 0, None, d_mv.data_ptr())),
        ("block_set", lambda: hip_ctx.inloop_subpel_search_dev(S, p.w, R, p.ref_geom[0], d_desc.data_ptr(), 1, 7, d_sad.data_ptr(), d_mv.data_ptr())),
        ("null", lambda: hip_ctx.inloop_fullpel_search_dev(S, p.w, R, p.ref_geom[0], None, 1, 0, d_sad.data_ptr(), d_mv.data_ptr())),
        ("block_set", lambda: hip_ctx.inloop_fullpel_search_dev(S, p.w, R, p.ref_geom[0], d_desc.data_ptr(), 1, -1, d_sad.data_ptr(), d_mv.data_ptr())),
        ("1..127", lambda: hip_ctx.inloop_area_dev(C, B, 1, p.w, p.h, p.src_geom, p.ref_geom, 128, 64, d_desc.data_ptr())),
        ("null", lambda: hip_ctx.inloop_area_dev(None, B, 1, p.w, p.h, p.src_geom, p.ref_geom, 64, 64, d_desc.data_ptr())),
        ("null", lambda: hip_ctx.inloop_pack_dev(None, 1, d_out.data_ptr())),
        ("border of 63", lambda: hip_ctx.inloop_area_dev(C, B, 1, p.w, p.h, p.src_geom, (p.ref_geom[0], 62, 64), 64, 64, d_desc.data_ptr())),
        ("border of 63", lambda: hip_ctx.inloop_area_dev(C, B, 1, p.w, p.h, p.src_geom, (p.ref_geom[0], 64, 0), 64, 64, d_desc.data_ptr())),
        ("border of 63", lambda: hip_ctx.inloop_area_dev(C, B, 1, p.w, p.h, p.src_geom, (p.w + 64 + 62, 64, 64), 64, 64, d_desc.data_ptr())),
        ("src_stride", lambda: hip_ctx.inloop_area_dev(C, B, 1, p.w, p.h, (p.w - 1, 0, 0), p.ref_geom, 64, 64, d_desc.data_ptr())),
        ("border of 63", lambda: hip_ctx.inloop_search_dev(S, p.src_geom, R, (p.ref_geom[0], 64, 62), p.w, p.h, C, B, 1, aw, ah, d_sad.data_ptr(), d_mv.data_ptr(),
                                                           d_out.data_ptr())),
        ("85 or 209", lambda: hip_ctx.inloop_centers_dev(S, 84, 0, 1, C)), ("list_index", lambda: hip_ctx.inloop_centers_dev(S, 85, 2, 1, C)),
    ]
    for text, call in refusals:
        with pytest.raises(svtav1_hip.SvtHipError) as e:
            call()
        assert text in str(e.value), (text, str(e.value))
    # the context still works
    search()
    hip_ctx.synchronize()
    assert np.array_equal(_host(d_sad, np.uint32, (1, iu.N_BLOCKS)), want["best_sad"][0])
