"""The coefficient-rate restatement (tests/rate_util.py) against the reference: the fixture tests/golden/coeff_rate.npz everywhere,
the reference's own Av1TuEstimateCoeffBits live where the reference and the oracle's objects exist; the candidate masks of the
library's svthip_tx_search_type_mask; the layout of svthip_coeff_rate_tables.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import rate_util
import svtav1_hip
from tq_util import RealTables

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "coeff_rate.npz")


@pytest.fixture(scope="module")
def fixture():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _tables(fx):
    return fx["tables"].view(svtav1_hip.COEFF_RATE_TABLES_DTYPE).reshape(-1)


def _n(ts):
    w, h = svtav1_hip.TX_SIZES_WH[ts]
    return min(w, 32) * min(h, 32)


def test_fixture_covers_the_ground(fixture):
    c = fixture["cases"]
    assert len(c) >= 2000 and _tables(fixture).shape == (4,)
    assert set(c["tx_size"]) == set(range(19)) and set(c["intra_mode"][c["is_inter"] == 0]) == set(range(13))
    assert set(c["plane_type"]) == {0, 1} and set(c["reduced_tx_set"]) == {0, 1} and set(c["txb_skip_ctx"]) == set(range(13))
    assert set(c["dc_sign_ctx"]) == {0, 1, 2} and set(c["table"]) == {0, 1, 2, 3}
    for ts in range(19):
        types = set(c["tx_type"][c["tx_size"] == ts])
        w, h = svtav1_hip.TX_SIZES_WH[ts]
        assert types == set(svtav1_hip.valid_tx_types(w, h)), ts
        eobs = set(c["eob"][c["tx_size"] == ts])
        assert {0, 1, 2, _n(ts)} <= eobs
    lv = np.abs(fixture["levels"].astype(np.int64))
    assert {3, 15, 127, 128} <= set(lv.tolist()) and lv.max() >= 1 << 14


def test_restatement_reproduces_the_fixture(fixture):
    tabs = RealTables()
    T = _tables(fixture)
    bad = []
    for c in fixture["cases"]:
        ts, tt = int(c["tx_size"]), int(c["tx_type"])
        n = _n(ts)
        o = tabs.scan_offset(ts, tt)
        got = rate_util.coeff_bits(T[c["table"]], fixture["levels"][c["level_offset"]:c["level_offset"] + n], tabs.iscan_pool[o:o + n],
                                   int(c["eob"]), ts, tt, int(c["plane_type"]), int(c["txb_skip_ctx"]), int(c["dc_sign_ctx"]), int(c["is_inter"]),
                                   int(c["intra_mode"]), int(c["reduced_tx_set"]))
        if got != int(c["bits"]):
            bad.append((dict(zip(fixture["cases"].dtype.names, c)), got))
    assert not bad, bad[:5]


def test_type_masks_match_the_reference(fixture):
    m = fixture["masks"]
    for ts in range(19):
        for inter in (0, 1):
            for red in (0, 1):
                for fast in (0, 1):
                    want = int(m[ts, inter, red, fast])
                    assert rate_util.tx_search_type_mask(ts, inter, red, fast) == want
                    assert svtav1_hip.tx_search_type_mask(ts, inter, red, fast) == want, (ts, inter, red, fast)
    assert all(svtav1_hip.tx_search_type_mask(ts, i, r, f) & 1 for ts in range(19) for i in (0, 1) for r in (0, 1) for f in (0, 1))


def test_tables_layout_matches_the_c_header(tmp_path):
    """svthip_coeff_rate_tables / svthip_coeff_rate_desc / search structs: the numpy and ctypes views have the C layout"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "svtav1_hip.h"\n'
                   "_Static_assert(sizeof(svthip_lv_map_coeff_cost) == 2116, \"coeff cost\");\n"
                   "_Static_assert(offsetof(svthip_lv_map_coeff_cost, lps_cost) == 256 * 4, \"lps\");\n"
                   "_Static_assert(sizeof(svthip_coeff_rate_tables) == 34088, \"tables\");\n"
                   "_Static_assert(offsetof(svthip_coeff_rate_tables, eobFracBits) == 21160, \"eob\");\n"
                   "_Static_assert(offsetof(svthip_coeff_rate_tables, interTxTypeFacBits) == 22392, \"inter\");\n"
                   "_Static_assert(offsetof(svthip_coeff_rate_tables, intraTxTypeFacBits) == 23480, \"intra\");\n"
                   "_Static_assert(sizeof(svthip_coeff_rate_desc) == 16, \"desc\");\n"
                   "_Static_assert(sizeof(svthip_tx_search_tu) == 40 && offsetof(svthip_tx_search_tu, type_mask) == 28, \"tu\");\n"
                   "_Static_assert(sizeof(svthip_tx_search_result) == 40 && offsetof(svthip_tx_search_result, candidate) == 32, \"res\");\n")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src)])
    d = svtav1_hip.COEFF_RATE_TABLES_DTYPE
    assert (d.itemsize, d.fields["eobFracBits"][1], d.fields["interTxTypeFacBits"][1], d.fields["intraTxTypeFacBits"][1]) == (34088, 21160, 22392, 23480)
    assert svtav1_hip.TxSearchTu.type_mask.offset == 28 and svtav1_hip.TxSearchResult.candidate.offset == 32


@pytest.fixture(scope="module")
def refdrv(tmp_path_factory):
    if not rate_util.reference_available():
        pytest.skip("reference sources / oracle/_ref/obj_all not present")
    return rate_util.build_reference_driver(str(tmp_path_factory.mktemp("ref_rate")))


def test_reference_struct_layout_pinned(refdrv):
    """the driver's _Static_asserts (sizeof / offsetof of the four fields against MdRateEstimationContext_t) compiled: it built"""
    assert refdrv.drv_init(100) == 0


def test_restatement_matches_live_reference(refdrv):
    tabs = RealTables()
    rng = np.random.default_rng(77)
    n_checked = 0
    for qi in (0, 45, 90, 255):
        T = rate_util.reference_tables(refdrv, qi, svtav1_hip.COEFF_RATE_TABLES_DTYPE)[0]
        for ts in range(19):
            w, h = svtav1_hip.TX_SIZES_WH[ts]
            n = _n(ts)
            for tt in svtav1_hip.valid_tx_types(w, h):
                o = tabs.scan_offset(ts, tt)
                iscan = tabs.iscan_pool[o:o + n]
                eob = int(rng.integers(0, n + 1))
                q = np.zeros(n, np.int64)
                scan = np.argsort(iscan)
                q[scan[:eob]] = rng.laplace(0, 3, eob).astype(np.int64) * rng.choice([1, 1, 1, 50], eob)
                if eob:
                    q[scan[eob - 1]] = int(rng.choice([-1, 1, 4, -300]))
                plane, skip, dcs, inter, mode, red = (int(rng.integers(0, 2)), int(rng.integers(0, 13)), int(rng.integers(0, 3)),
                                                      int(rng.integers(0, 2)), int(rng.integers(0, 13)), int(rng.integers(0, 2)))
                lv = np.ascontiguousarray(q.astype(np.int32))
                want = int(refdrv.drv_bits(lv.ctypes.data, eob, plane, ts, tt, skip, dcs, inter, mode, red))
                assert rate_util.coeff_bits(T, q, iscan, eob, ts, tt, plane, skip, dcs, inter, mode, red) == want, (qi, ts, tt, eob)
                n_checked += 1
    assert n_checked > 500
