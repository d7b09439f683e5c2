"""GPU parity of the search-centre kernel at the shapes its specialised paths take: level 0 in one band (1080p, 200 %) and in bands
(4K, the 350 / 525 % multipliers), the fixed-shape level-1 / level-2 loops (full SBs, unclipped 16 x 16 / 8 x 8 areas) next to the
general ones (partial SBs, clipped windows), and CheckZeroZeroCenter with and without level 2.  Descriptors and centres are compared
bit-exactly with the oracle for every SB, the full-pel results on a sample of SBs (as tests/test_hme_gpu.py does at 1080p)."""
import numpy as np
import pytest

import svtav1_hip
from test_hme_gpu import DeviceChain, _pics

pytestmark = pytest.mark.gpu


def _run_and_check(hip_ctx, oracle, pics, P, two_lists, n_sample=24):
    chain = DeviceChain(hip_ctx, pics)
    dev = chain.run(P, two_lists)
    n = chain.n
    sample = np.sort(np.random.default_rng(11).choice(n, min(n, n_sample), replace=False))
    pool, descs = svtav1_hip.build_picture_pool(pics)
    sb = chain.sb
    state = np.zeros((n, 25), np.int16)
    mv0 = None
    for l in range(2 if two_lists else 1):
        d, c = oracle.hme_search_center_batch(pool, descs[0], descs[1 + l], P, l, sb, mv0, state)
        for name, a, b in (("desc", dev[l][0], d), ("center", dev[l][1], c)):
            bad = np.argwhere(a != b)
            assert bad.size == 0, f"list {l} {name}: {len(bad)} mismatches, first at {bad[0]}: hip {a[tuple(bad[0])]} oracle {b[tuple(bad[0])]}"
        s, m = oracle.fullpel_search_batch(pool, pool, d[sample], descs[0].full_stride, descs[1 + l].full_stride)
        assert np.array_equal(dev[l][2][sample], s), f"list {l} sad"
        assert np.array_equal(dev[l][3][sample], m), f"list {l} mv"
        # list 1's direct candidate reads list 0's best 64x64 vector: the device's, checked above on the sample and equal to the
        # oracle's wherever the descriptors are (the full-pel search is pinned by its own tests)
        mv0 = np.ascontiguousarray(dev[l][3][:, 0])
    return dev


CASES = [
    # (w, h, content, hierarchy, temporal layer, two lists, ref_poc_equal)
    (1920, 1080, "synth", 3, 0, False, False),   # headline shape: level 0 in one band, fixed-shape levels 1 / 2
    (1920, 1080, "synth", 3, 1, True, False),    # 140 %: level-0 width 67 (not a multiple of 16), both lists with l0_best_mv64
    (1920, 1080, "synth", 3, 1, True, True),     # the ref_poc_equal sort picks the centre of list 1
    (1920, 1080, "synth", 4, 0, False, False),   # 350 %: level 0 in bands
    (1920, 1080, "synth", 5, 0, False, False),   # 525 %
    (1000, 600, "pan", 3, 1, True, True),        # partial SBs, clipped level-1 / level-2 windows
    (1920, 1080, "flat", 3, 0, False, False),    # ties everywhere: the strict raster rule at every level
    (1920, 1080, "flat", 3, 1, True, True),
]


@pytest.mark.parametrize("case", CASES)
def test_hme_shapes_match_oracle(hip_ctx, oracle, case):
    pytest.importorskip("torch")
    w, h, kind, hier, tl, two, poc_eq = case
    pics = _pics(w, h, kind)
    P = svtav1_hip.default_me_params(w, h, hier, tl, True, poc_eq)
    _run_and_check(hip_ctx, oracle, pics, P, two)


def test_hme_4k_multiband_level0(hip_ctx, oracle):
    pytest.importorskip("torch")
    pics = _pics(3840, 2160, "synth")
    P = svtav1_hip.default_me_params(3840, 2160, 3, 0)
    _run_and_check(hip_ctx, oracle, pics, P, False)


@pytest.mark.parametrize("flags", [(1, 1, 0), (1, 0, 1), (0, 1, 1)])
def test_hme_zero_centre_check_without_level2(hip_ctx, oracle, flags):
    """CheckZeroZeroCenter takes its two SADs from the centre check and level 2 only when level 2 ran; otherwise it computes them."""
    pytest.importorskip("torch")
    pics = _pics(1920, 1080, "pan")
    P = svtav1_hip.default_me_params(1920, 1080, 3, 1, True, True)
    P.enable_hme_level0_flag, P.enable_hme_level1_flag, P.enable_hme_level2_flag = flags
    dev = _run_and_check(hip_ctx, oracle, pics, P, True)
    assert (dev[0][1] != 0).any()


def test_hme_1080p_batched_equals_per_picture(hip_ctx):
    """The batched entry over several 1080p picture pairs == one per-picture launch per pair, at the headline shape."""
    import torch
    from svtav1_hip import synth

    w, h, n_pic = 1920, 1080, 3
    pics = [synth.PaPicture(synth.synth_luma(w, h, 3 * i)) for i in range(n_pic + 1)]
    pool, pd = svtav1_hip.build_picture_pool(pics)
    d_pool = torch.from_numpy(np.concatenate([pool, np.zeros(64, np.uint8)])).to("cuda:0")
    sbs = svtav1_hip.sb_origins(w, h)
    n_sb = sbs.shape[0]
    d_sb = torch.from_numpy(sbs.view(np.int16).copy()).to("cuda:0")
    params = svtav1_hip.default_me_params(w, h, 3, 0)
    d_one = torch.zeros((n_pic * n_sb, 6), dtype=torch.int32, device="cuda:0")
    d_cen1 = torch.zeros((n_pic * n_sb, 2), dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    for i in range(n_pic):
        hip_ctx.hme_search_center_dev(d_pool.data_ptr(), pd[i + 1], pd[i], params, 0, d_sb.data_ptr(), n_sb, None,
                                      d_one.data_ptr() + i * n_sb * 24, d_cen1.data_ptr() + i * n_sb * 4)
    d_bat = torch.zeros((n_pic * n_sb, 6), dtype=torch.int32, device="cuda:0")
    d_cen2 = torch.zeros((n_pic * n_sb, 2), dtype=torch.int16, device="cuda:0")
    hip_ctx.synchronize()
    hip_ctx.hme_search_center_batch_dev(d_pool.data_ptr(), [pd[i + 1] for i in range(n_pic)], [pd[i] for i in range(n_pic)], params, 0,
                                        d_sb.data_ptr(), n_sb, None, d_bat.data_ptr(), d_cen2.data_ptr())
    hip_ctx.synchronize()
    assert torch.equal(d_one, d_bat) and torch.equal(d_cen1, d_cen2)
    assert (d_cen2 != 0).any()
