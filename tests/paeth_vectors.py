"""TEST INFRASTRUCTURE: PAETH_PRED worked sample by sample from the rule of the AV1 specification (7.11.2.2), in plain Python loops that
share nothing with intra_pred_util.predict_from_edges.  The reference assigns no PAETH predictor, so these vectors are what pins mode 12:
the restatement (CPU test) and the device (GPU test) must both reproduce them.  Edges are not constant (noise, noisy ramps, the extremes
0 and the maximum), sizes are square, wide, tall and multi-pass, both depths."""
import numpy as np

import intra_pred_util as iu

SIZES = (0, 1, 14, 13, 16, 4)   # 4x4, 8x8, 16x4, 4x16, 32x8, 64x64
N_PER_SIZE = 9


def paeth_block(above, left, topleft, w, h, winners):
    out = [[0] * w for _ in range(h)]
    for r in range(h):
        for c in range(w):
            base = above[c] + left[r] - topleft
            p_left, p_top, p_tl = abs(base - left[r]), abs(base - above[c]), abs(base - topleft)
            if p_left <= p_top and p_left <= p_tl:
                name, v, others = "left", left[r], (above[c], topleft)
            elif p_top <= p_tl:
                name, v, others = "top", above[c], (left[r], topleft)
            else:
                name, v, others = "topleft", topleft, (left[r], above[c])
            if v not in others:          # the winner shows in the output
                winners.add(name)
            out[r][c] = v
    return out


def vectors(tx_size, bd):
    """(edge, desc, want, winners): N_PER_SIZE blocks of mode 12 with whole edges, in iu.random_case's layout"""
    w, h = iu.TX_SIZES_WH[tx_size]
    edge, desc, _ = iu.random_case(np.random.default_rng(1200 + 10 * tx_size + bd), N_PER_SIZE, tx_size, bd)
    desc["mode"], desc["angle_delta"] = iu.PAETH, 0
    desc["n_top_px"], desc["n_left_px"], desc["n_topright_px"], desc["n_bottomleft_px"] = w, h, 0, 0
    winners = set()
    want = np.zeros((N_PER_SIZE, h, w), edge.dtype)
    for i, d in enumerate(desc):
        ao, lo = int(d["above_offset"]), int(d["left_offset"])
        above = [int(v) for v in edge[ao:ao + w]]
        left = [int(v) for v in edge[lo:lo + h]]
        want[i] = paeth_block(above, left, int(edge[ao - 1]), w, h, winners)
    return edge, desc, want.reshape(-1), winners
