"""GPU parity of the search-centre kernel at level-1 / level-2 areas that no default parameter set has (every default is 16 x 16 and
8 x 8): the two decisions of the level dispatch in me_hme_impl.h that the other HME tests do not reach.
  * Level 1 with 80 x 64 areas: 5120 positions, more than the 4096 a 32-bit (sad << 12 | position) key holds, so the LDS loop runs with
    its 64-bit key.  The 32 x 16-row block over an 80-wide area has a window pitch of 29 dwords; 61 rows fit the 7 KB slice, 30 of
    them below the band, so the 64 search rows run in three bands of 31, 31 and 2.
  * Level 2 with 48 x 8 areas: 384 positions would take the 32-bit key, but the 64 x 32-row block needs 62 window rows beyond the band
    and a 48-wide area (pitch 29 dwords again) leaves 61: no band fits, so every full SB with an unclipped width takes the generic loop.
640 x 384 is 60 SBs, all full.  `flat` makes every position a tie, so the strict raster rule has to hold across the bands.
Descriptors and centres are compared bit for bit with the oracle for every SB, with the checking pattern of test_hme_shapes_gpu.py."""
import pytest

import svtav1_hip
from test_hme_gpu import _pics
from test_hme_shapes_gpu import _run_and_check

pytestmark = pytest.mark.gpu

SIZE = (640, 384)


def _params():
    P = svtav1_hip.default_me_params(SIZE[0], SIZE[1], 3, 0)
    for k in range(2):
        P.hme_level1_search_area_in_width_array[k], P.hme_level1_search_area_in_height_array[k] = 80, 64
        P.hme_level2_search_area_in_width_array[k], P.hme_level2_search_area_in_height_array[k] = 48, 8
    return P


@pytest.mark.parametrize("kind", ["synth", "flat"])
def test_hme_wide_levels_match_oracle(hip_ctx, oracle, kind):
    pytest.importorskip("torch")
    _run_and_check(hip_ctx, oracle, _pics(SIZE[0], SIZE[1], kind), _params(), False)
