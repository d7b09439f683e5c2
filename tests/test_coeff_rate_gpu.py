"""svthip_coeff_rate_batch_dev (tq_coeff_rate.hip) bit-exact against the reference's bits in tests/golden/coeff_rate.npz and against
the restatement tests/rate_util.py on random batches of every size (small TUs packed several to a wave, partial last waves)."""
import numpy as np
import pytest

import rate_util
import svtav1_hip
from tq_util import RealTables

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _n(ts):
    w, h = svtav1_hip.TX_SIZES_WH[ts]
    return min(w, 32) * min(h, 32)


def _run(ctx, d_tables, tables_index, q_pool, eobs, desc, ts, d_iscan):
    import torch
    d_q, d_eob, d_desc = _dev(q_pool.astype(np.int32)), _dev(eobs.astype(np.uint16)), _dev(desc)
    d_bits = torch.zeros(len(desc), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.coeff_rate_batch_dev(d_tables.data_ptr() + tables_index * svtav1_hip.COEFF_RATE_TABLES_DTYPE.itemsize, d_q.data_ptr(), d_eob.data_ptr(),
                             d_iscan.data_ptr(), d_desc.data_ptr(), len(desc), ts, d_bits.data_ptr())
    ctx.synchronize()
    return d_bits.cpu().numpy().view(np.uint32)


def test_rate_kernel_matches_reference_fixture(hip_ctx):
    pytest.importorskip("torch")
    z = np.load(rate_util.os.path.join(rate_util.ROOT, "tests", "golden", "coeff_rate.npz"))
    cases, levels = z["cases"], z["levels"]
    tabs = RealTables()
    d_tables, d_iscan = _dev(z["tables"]), _dev(tabs.iscan_pool)
    n_checked = 0
    for ts in range(19):
        for ti in range(4):
            sel = cases[(cases["tx_size"] == ts) & (cases["table"] == ti)]
            if not len(sel):
                continue
            n = _n(ts)
            pool = np.concatenate([levels[c["level_offset"]:c["level_offset"] + n].astype(np.int32) for c in sel])
            desc = np.zeros(len(sel), svtav1_hip.COEFF_RATE_DESC_DTYPE)
            desc["coeff_offset"] = np.arange(len(sel)) * n
            desc["iscan_offset"] = [tabs.scan_offset(ts, int(t)) for t in sel["tx_type"]]
            for f in ("tx_type", "plane_type", "txb_skip_ctx", "dc_sign_ctx", "is_inter", "intra_mode", "reduced_tx_set"):
                desc[f] = sel[f]
            got = _run(hip_ctx, d_tables, ti, pool, sel["eob"], desc, ts, d_iscan)
            bad = np.nonzero(got != sel["bits"].astype(np.uint32))[0]
            assert not len(bad), (ts, ti, [(dict(zip(cases.dtype.names, sel[i])), int(got[i])) for i in bad[:3]])
            n_checked += len(sel)
    assert n_checked == len(cases)


def _random_batch(rng, ts, n_tu, tabs):
    n = _n(ts)
    w, h = svtav1_hip.TX_SIZES_WH[ts]
    types = svtav1_hip.valid_tx_types(w, h)
    pool = np.zeros(n_tu * n, np.int32)
    desc = np.zeros(n_tu, svtav1_hip.COEFF_RATE_DESC_DTYPE)
    eobs = np.zeros(n_tu, np.int64)
    for i in range(n_tu):
        tt = types[int(rng.integers(0, len(types)))]
        o = tabs.scan_offset(ts, tt)
        scan = np.argsort(tabs.iscan_pool[o:o + n])
        k = i % 5
        eob = 0 if k == 0 else 1 if k == 1 else n if k == 2 else int(rng.integers(1, n + 1))
        q = np.zeros(n, np.int64)
        q[scan[:eob]] = rng.laplace(0, [1, 2, 6, 40, 3][k], eob).astype(np.int64) * rng.choice([1, 1, 1, 1, 300], eob)
        if eob:
            q[scan[eob - 1]] = int(rng.choice([1, -1, 2, -15, 20000]))
        pool[i * n:(i + 1) * n] = q
        desc[i] = (i * n, o, tt, int(rng.integers(0, 2)), int(rng.integers(0, 13)), int(rng.integers(0, 3)), int(rng.integers(0, 2)),
                   int(rng.integers(0, 13)), int(rng.integers(0, 2)), 0)
        eobs[i] = eob
    return pool, eobs, desc


@pytest.mark.parametrize("ts", range(19))
def test_rate_kernel_matches_restatement(hip_ctx, ts):
    """every size; batch lengths that leave partial waves and partial workgroups (small sizes: 4 / 8 / 16 TUs share a wave)"""
    pytest.importorskip("torch")
    z = np.load(rate_util.os.path.join(rate_util.ROOT, "tests", "golden", "coeff_rate.npz"))
    T = z["tables"].view(svtav1_hip.COEFF_RATE_TABLES_DTYPE).reshape(-1)
    tabs = RealTables()
    rng = np.random.default_rng(100 + ts)
    n_tu = {16: 203, 32: 141, 64: 77}.get(_n(ts), 37)
    pool, eobs, desc = _random_batch(rng, ts, n_tu, tabs)
    got = _run(hip_ctx, _dev(z["tables"]), 2, pool, eobs, desc, ts, _dev(tabs.iscan_pool))
    n = _n(ts)
    for i, d in enumerate(desc):
        o = int(d["iscan_offset"])
        want = rate_util.coeff_bits(T[2], pool[i * n:(i + 1) * n], tabs.iscan_pool[o:o + n], int(eobs[i]), ts, int(d["tx_type"]), int(d["plane_type"]),
                                    int(d["txb_skip_ctx"]), int(d["dc_sign_ctx"]), int(d["is_inter"]), int(d["intra_mode"]), int(d["reduced_tx_set"]))
        assert int(got[i]) == want, (ts, i, dict(zip(desc.dtype.names, d)), int(eobs[i]))


def test_rate_kernel_refuses_bad_parameters(hip_ctx):
    torch = pytest.importorskip("torch")
    buf = torch.zeros(1 << 16, dtype=torch.int32, device="cuda:0")
    p = buf.data_ptr()
    with pytest.raises(svtav1_hip.SvtHipError):
        hip_ctx.coeff_rate_batch_dev(p, p, p, p, p, 1, 19, p)              # no such TxSize
    with pytest.raises(svtav1_hip.SvtHipError):
        hip_ctx.coeff_rate_batch_dev(p, p + 4, p, p, p, 1, 0, p)           # level pool not 16-byte aligned
    with pytest.raises(svtav1_hip.SvtHipError):
        hip_ctx.coeff_rate_batch_dev(p, p, p, p + 2, p, 1, 0, p)           # iscan pool not 8-byte aligned
    # a descriptor offset that is not a multiple of 4: that TU is refused in its output, its neighbours are computed
    z = np.load(rate_util.os.path.join(rate_util.ROOT, "tests", "golden", "coeff_rate.npz"))
    tabs = RealTables()
    pool, eobs, desc = _random_batch(np.random.default_rng(5), 1, 8, tabs)
    desc[3]["coeff_offset"] += 2
    got = _run(hip_ctx, _dev(z["tables"]), 0, np.concatenate([pool, np.zeros(64, np.int32)]), eobs, desc, 1, _dev(tabs.iscan_pool))
    assert got[3] == 0xffffffff and (got[[0, 1, 2, 4, 5, 6, 7]] != 0xffffffff).all()
