"""GPU: intra prediction and whole-PU inter prediction interleaved on one context (they share the refusal counter), with a reserve for a
large picture in between: results unchanged by the order of the calls."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import inter_pred_util as ipu  # noqa: E402
import intra_pred_util as iu  # noqa: E402
import svtav1_hip  # noqa: E402

pytestmark = pytest.mark.gpu


def test_intra_and_inter_calls_interleaved():
    pytest.importorskip("torch")
    ctx = svtav1_hip.Context(0)
    try:
        intra = {}
        for tx_size, bd in ((0, 8), (3, 8), (8, 10), (4, 10)):
            txw, txh = iu.TX_SIZES_WH[tx_size]
            edge, desc, _ = iu.random_case(np.random.default_rng(400 + tx_size), 45, tx_size, bd)
            want = np.full(45 * txw * txh, iu.FILL[bd], edge.dtype)
            assert iu.predict(edge, want, desc, tx_size, bd)[0] == 0
            intra[(tx_size, bd)] = (edge, desc, want)
        rng = np.random.default_rng(9)
        blank = lambda: ipu.Picture(np.full((256, 512), 0x55, np.uint8), np.full((128, 256), 0x55, np.uint8), np.full((128, 256), 0x55, np.uint8), 0)  # noqa: E731
        trefs = [ipu.random_picture(rng, 512, 256, ipu.border_for(16, 16), 8, kind) for kind in ("noise", "smooth")]
        tdesc = ipu.random_descs(rng, 300, 16, 16, 512, 256)
        twant = blank()
        assert ipu.predict(trefs[0], trefs[1], twant, tdesc, 16, 16, 8) == 0

        def run_intra(key, step):
            edge, desc, want = intra[key]
            got, _ = iu.run_device(ctx, edge, np.full_like(want, iu.FILL[key[1]]), desc, key[0], key[1])
            assert np.array_equal(got, want), (step, key)

        def run_inter(step):
            got, _ = ipu.run_device(ctx, trefs[0], trefs[1], blank(), tdesc, 16, 16, 8)
            for p in ("y", "cb", "cr"):
                assert np.array_equal(getattr(got, p), getattr(twant, p)), (step, p)

        keys = list(intra)
        run_intra(keys[0], "first")            # the refusal counter is created by an intra call
        run_inter("after an intra call")
        run_intra(keys[1], "after an inter call")
        ctx.reserve(3840, 2160, 85, 1, host_forms=True)
        run_intra(keys[2], "after the 4K reserve")
        run_inter("after the 4K reserve")
        run_intra(keys[3], "large blocks")
        run_intra(keys[0], "small again")
        run_inter("last")
        assert ctx.inter_pred_refused() == 0
    finally:
        ctx.close()
