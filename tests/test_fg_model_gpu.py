"""GPU: film-grain estimation (svthip_[highbd_]film_grain_noise_model_dev, svthip_film_grain_flat_block_tables_dev,
svthip_[highbd_]film_grain_flat_block_features_dev) through the C ABI against the reference's fixture (tests/golden/fg_model.npz): every
double of every case compared as bits (view(uint64) equality), plus status and counters.  Every plane sits inside a larger buffer with a
stride above its width; the output buffers are longer than what the entry may write and their tails are checked.  One chain per picture:
features on the device, numpy's finish, the model on the device with that map, against the reference's aom_flat_block_finder_run and
aom_noise_model_update on the same picture."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import fg_model_util as mu  # noqa: E402
import svtav1_hip  # noqa: E402

pytestmark = pytest.mark.gpu
TAIL = 64


class _Picture:
    """data and denoised planes inside garbage on the device, strides above the widths"""

    def __init__(self, torch, data, den, bd):
        self.torch, self.bd = torch, bd
        self.h, self.w = data[0].shape
        rng = np.random.default_rng(5)
        self.keep, self.ptrs, self.stride = [], [[], []], []
        for which, planes in enumerate((data, den)):
            for k, p in enumerate(planes):
                ph, pw = p.shape
                stride = pw + 6 + 2 * k
                buf = rng.integers(0, 1 << bd, (ph + 4, stride)).astype(p.dtype)
                buf[2:2 + ph, 4:4 + pw] = p
                t = torch.from_numpy(buf.view(np.uint8).reshape(-1).copy()).to("cuda:0")
                self.keep.append(t)
                self.ptrs[which].append(t.data_ptr() + (2 * stride + 4) * p.dtype.itemsize)
                if not which:
                    self.stride.append(stride)
        torch.cuda.synchronize()

    def model(self, ctx, flat):
        torch = self.torch
        d_flat = torch.from_numpy(np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1).copy()).to("cuda:0")
        d_state = torch.full((mu.STATE.itemsize + TAIL,), 0x5A, dtype=torch.uint8, device="cuda:0")
        a = (self.ptrs[0], self.ptrs[1], self.stride, self.w, self.h)
        if self.bd == 8:
            ctx.film_grain_noise_model_dev(*a, d_flat.data_ptr(), d_state.data_ptr())
        else:
            ctx.highbd_film_grain_noise_model_dev(*a, self.bd, d_flat.data_ptr(), d_state.data_ptr())
        ctx.synchronize()
        raw = d_state.cpu().numpy()
        assert (raw[mu.STATE.itemsize:] == 0x5A).all(), "written behind the state"
        return np.frombuffer(raw[:mu.STATE.itemsize].tobytes(), mu.STATE)[0]

    def features(self, ctx, d_tables=None):
        torch = self.torch
        nb = int(np.prod(mu.blocks_of(self.w, self.h)))
        d_feat = torch.full((nb * mu.FEATURES.itemsize + TAIL,), 0x5A, dtype=torch.uint8, device="cuda:0")
        d_is = torch.full((nb + TAIL,), 0x5A, dtype=torch.uint8, device="cuda:0")
        a = (self.ptrs[0][0], self.stride[0], self.w, self.h)
        if self.bd == 8:
            ctx.film_grain_flat_block_features_dev(*a, d_feat.data_ptr(), d_is.data_ptr(), d_tables)
        else:
            ctx.highbd_film_grain_flat_block_features_dev(*a, self.bd, d_feat.data_ptr(), d_is.data_ptr(), d_tables)
        ctx.synchronize()
        feat, is_flat = d_feat.cpu().numpy(), d_is.cpu().numpy()
        assert (feat[nb * mu.FEATURES.itemsize:] == 0x5A).all() and (is_flat[nb:] == 0x5A).all(), "written behind the outputs"
        return np.frombuffer(feat[:nb * mu.FEATURES.itemsize].tobytes(), mu.FEATURES), is_flat[:nb]


def _assert_same_state(got, want, what):
    for which in ("latest", "combined"):
        for c in range(3):
            for f in got[which].dtype.names:
                a, b = np.atleast_1d(got[which][c][f]), np.atleast_1d(want[which][c][f])
                if a.dtype == np.float64:
                    a, b = a.view(np.uint64), b.view(np.uint64)
                assert np.array_equal(a, b), (what, which, c, f, np.flatnonzero(a != b)[:6])
    assert got["status"] == want["status"] and got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("k", range(len(mu.CASES)))
def test_noise_model_matches_reference(hip_ctx, k):
    torch = pytest.importorskip("torch")
    p, kind, variant = mu.CASES[k]
    data, den = mu.planes_of(p, variant)
    pic = _Picture(torch, data, den, mu.PICTURES[p][2])
    got = pic.model(hip_ctx, mu.flat_map(p, kind))
    _assert_same_state(got, np.frombuffer(mu.fixture()[f"state_{k}"].tobytes(), mu.STATE)[0], mu.CASES[k])


def test_flat_block_tables_match_reference(hip_ctx):
    torch = pytest.importorskip("torch")
    d = torch.full((mu.TABLES_DOUBLES * 8 + TAIL,), 0x5A, dtype=torch.uint8, device="cuda:0")
    hip_ctx.film_grain_flat_block_tables_dev(d.data_ptr())
    hip_ctx.synchronize()
    raw = d.cpu().numpy()
    assert (raw[mu.TABLES_DOUBLES * 8:] == 0x5A).all()
    assert np.array_equal(raw[:mu.TABLES_DOUBLES * 8].view(np.uint64), mu.fixture()["tables"].view(np.uint64))


@pytest.mark.parametrize("p", range(len(mu.PICTURES)))
def test_flat_block_features_and_chain_match_reference(hip_ctx, p):
    """features with the tables built in scratch and with given tables; then numpy's finish and the model with that map"""
    torch = pytest.importorskip("torch")
    fx = mu.fixture()
    w, h, bd = mu.PICTURES[p]
    data, den = mu.planes_of(p)
    pic = _Picture(torch, data, den, bd)
    want = np.frombuffer(fx[f"features_{p}"].tobytes(), mu.FEATURES)
    d_tables = torch.from_numpy(fx["tables"].copy()).to("cuda:0")
    for tables in (None, d_tables.data_ptr()):
        feat, is_flat = pic.features(hip_ctx, tables)
        for f in mu.FEATURES.names:
            assert np.array_equal(feat[f].view(np.uint64), want[f].view(np.uint64)), (p, f, np.flatnonzero(feat[f] != want[f])[:6])
        assert np.array_equal(is_flat, fx[f"is_flat_{p}"]), p
    final, _, _ = mu.finish_flat_blocks(feat, is_flat)
    assert np.array_equal(final, fx[f"final_{p}"]), "the finish of the device's features differs from aom_flat_block_finder_run"
    got = pic.model(hip_ctx, final)
    _assert_same_state(got, np.frombuffer(fx[f"chain_{p}"].tobytes(), mu.STATE)[0], ("chain", p))


def test_two_models_on_one_context_leave_nothing_stale():
    """different sizes and depths through one context's scratch, in both orders"""
    torch = pytest.importorskip("torch")
    fx = mu.fixture()
    ctx = svtav1_hip.Context(0)
    try:
        for k in (5, 9, 2, 5, 3, 9):
            p, kind, variant = mu.CASES[k]
            data, den = mu.planes_of(p, variant)
            got = _Picture(torch, data, den, mu.PICTURES[p][2]).model(ctx, mu.flat_map(p, kind))
            _assert_same_state(got, np.frombuffer(fx[f"state_{k}"].tobytes(), mu.STATE)[0], k)
    finally:
        ctx.close()
