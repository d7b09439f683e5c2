"""GPU: the motion-analysis entries at the end of the device's own front end.  On a 256x256 pair of synthetic pictures shifted by a global pan:
svthip_pa_derive_planes_dev -> svthip_pa_block_stats_dev -> svthip_motion_estimate_batch_dev -> svthip_open_loop_intra_search_batch_dev -> the
five svthip_ma_*_dev entries, all enqueued on one stream with no host copy and no synchronisation in between.  Afterwards the ME rows, the
OIS words and the statistics tables are downloaded and the five results are compared with the restatement (tests/ma_stats_util.py) fed those
tables.  The pan must be detected."""
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


def test_front_end_chain_detects_the_pan(hip_ctx):
    torch = pytest.importorskip("torch")
    ctx, w, h = hip_ctx, 256, 256
    cur, ref = mu.pan_pair(w, h)
    n_sb = mu.n_sbs(w, h)
    # the pool: [ref, cur] with interiors only, then their chroma planes
    laid_out, descs = svtav1_hip.build_picture_pool([synth.PaPicture(ref), synth.PaPicture(cur)])
    cstride, luma_bytes = w // 2, laid_out.size
    pool = np.full(luma_bytes + 4 * cstride * (h // 2) + 256, 0xEE, np.uint8)
    offsets = []
    for j, (luma, d) in enumerate(zip((ref, cur), descs)):
        pool[d.full_offset:d.full_offset + d.full_stride * (h + 136)].reshape(h + 136, d.full_stride)[68:68 + h, 68:68 + w] = luma
        pair = [luma_bytes + (2 * j + c) * cstride * (h // 2) for c in (0, 1)]
        for at, plane in zip(pair, (luma[::2, ::2], 255 - luma[1::2, 1::2])):
            pool[at:at + cstride * (h // 2)] = plane.reshape(-1)
        offsets.append(pair)
    d_pool = torch.from_numpy(pool).to("cuda:0")
    d_sb = torch.from_numpy(svtav1_hip.sb_origins(w, h).view(np.int16).copy()).to("cuda:0")
    z = lambda shape, t: torch.zeros(shape, dtype=t, device="cuda:0")  # noqa: E731
    d_y, d_v, d_cb, d_cr = z((2, n_sb, 85), torch.uint8), z((2, n_sb, 85), torch.int16), z((2, n_sb, 21), torch.uint8), z((2, n_sb, 21), torch.uint8)
    d_me, d_cand, d_total = z((n_sb, 85, 24), torch.uint8), z((n_sb, 85, 18), torch.int32), z((n_sb, 85), torch.uint8)
    d_sad, d_zz, d_nm = z((n_sb,), torch.int32), z((n_sb,), torch.uint8), z((n_sb,), torch.uint8)
    d_energy, d_mean = z((2, n_sb, 5), torch.int64), z((2, n_sb, 5), torch.int64)
    d_rc, d_inter, d_intra, d_hist, d_full = z((n_sb,), torch.int32), z((n_sb,), torch.int32), z((n_sb,), torch.int32), z((2, 128), torch.int32), z((1,), torch.int32)
    d_gm, d_flags = z((12,), torch.int32), z((n_sb, 4), torch.uint8)
    torch.cuda.synchronize()

    P = svtav1_hip.default_me_params(w, h, 3, 0)
    ois = svtav1_hip.OisParams()
    ois.temporal_layer_index, ois.is_used_as_reference_flag = 0, 1
    signals = dict(slice_is_intra=0, temporal_layer_index=0, hierarchical_levels=3, is_used_as_reference_flag=1, intensity_transition_flag=0)
    inter = [svtav1_hip.make_ma_params(**signals, ref_index=0)]
    both = [svtav1_hip.make_ma_params(slice_is_intra=1), inter[0]]      # the reference picture as the intra picture it was, then the current one
    p = d_pool.data_ptr()
    cur_y, cur_v = d_y.data_ptr() + n_sb * 85, d_v.data_ptr() + 2 * n_sb * 85
    # ---- the front end and the five entries, back to back on the context's stream
    ctx.pa_derive_planes_dev(p, descs)
    ctx.pa_block_stats_dev(p, descs, offsets, cstride, 0, d_y.data_ptr(), d_v.data_ptr(), d_cb.data_ptr(), d_cr.data_ptr())
    ctx.motion_estimate_batch_dev(p, descs[1:], descs[:1], None, P, d_sb.data_ptr(), n_sb, d_me.data_ptr(), True, 0)
    ctx.open_loop_intra_search_batch_dev(p, descs[1:], ois, d_sb.data_ptr(), n_sb, d_me.data_ptr(), 85, d_cand.data_ptr(), d_total.data_ptr())
    ctx.ma_zz_sad_dev(p, descs[1:], descs[:1], d_sad.data_ptr(), d_zz.data_ptr(), d_nm.data_ptr())
    ctx.ma_ac_energy_dev(p, descs, both, d_y.data_ptr(), d_energy.data_ptr(), d_mean.data_ptr())
    ctx.ma_distortion_stats_dev(d_me.data_ptr(), 85, d_cand.data_ptr(), w, h, inter, d_rc.data_ptr(), d_inter.data_ptr(), d_intra.data_ptr(), d_hist.data_ptr(),
                                d_full.data_ptr())
    ctx.ma_global_motion_dev(d_me.data_ptr(), 85, w, h, inter, d_gm.data_ptr())
    ctx.ma_sb_flags_dev(cur_y, cur_v, d_y.data_ptr(), d_v.data_ptr(), 85, 2, d_me.data_ptr(), 85, d_cand.data_ptr(), w, h, inter, d_flags.data_ptr())
    ctx.synchronize()

    # ---- the restatement on the downloaded tables
    me = d_me.cpu().numpy().reshape(-1).view(mu.ME_DTYPE).reshape(n_sb, 85)
    cand = d_cand.cpu().numpy().view(np.uint32)
    y_mean, variance = d_y.cpu().numpy(), d_v.cpu().numpy().view(np.uint16)
    sad, zz, nm = mu.zz_sad(cur, ref)
    assert np.array_equal(d_sad.cpu().numpy().view(np.uint32), sad) and np.array_equal(d_zz.cpu().numpy(), zz) and np.array_equal(d_nm.cpu().numpy(), nm)
    assert sad.min() > 0                                   # the pictures differ on the 4-grid
    energy, mean = d_energy.cpu().numpy().view(np.uint64), d_mean.cpu().numpy().view(np.uint64)
    want_e, want_m = mu.ac_energy(ref, 1, y_mean[0])
    assert np.array_equal(energy[0], want_e) and np.array_equal(mean[0], want_m) and (energy[0] < mu.SENTINEL).all()
    assert (energy[1] == mu.SENTINEL).all() and (mean[1] == mu.SENTINEL).all()
    rc, inter_i, intra_i, hist, full = mu.distortion_stats(me, cand, w, h, 0)
    for got, want in ((d_rc, rc), (d_inter, inter_i), (d_intra, intra_i), (d_hist, hist), (d_full, full)):
        assert np.array_equal(got.cpu().numpy().view(np.uint32).reshape(np.shape(want)), want)
    assert int(full) == 16 and rc.max() > 0 and intra_i.max() > 0
    gm = d_gm.cpu().numpy()
    assert np.array_equal(gm, mu.global_motion(me, w, h, signals))
    assert gm[0] == 1 and gm[1] == 0 and gm[11] == 0 and abs(int(gm[2])) == 20 and gm[6] == 16 and gm[7] >= 13      # is_pan, 5 samples = 20 quarter samples
    flags = d_flags.cpu().numpy()
    assert np.array_equal(flags, mu.sb_flags(y_mean[1], variance[1], y_mean[0, :, 0], variance[0, :, 0], me, cand, w, h, signals))
