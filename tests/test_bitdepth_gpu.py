"""GPU: the five entries of the 10-bit picture forms, bit-exact against the reference's fixture (tests/golden/bitdepth.npz) at 72x40 and 136x72
with 1 and 3 pictures a call.  Every plane set lies in one flat buffer at offsets and strides that are no multiples of 16 bytes
(bitdepth_util.PlaneSet), filled with a guard value everywhere outside the interiors: after every call that writes, the bytes between width
and stride and around the planes are checked untouched.  Also: unpack without the 2-bit destination, unpack over a padded reference, sums
that need more than 32 bits, and the validators."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "svt-av1-1_amd", "python")]

import bitdepth_util as bu  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [(c, n) for c in range(len(bu.CASES)) for n in (1, 3)]
BAD_PARAMETER = "80001005"


@pytest.fixture(scope="module")
def ctx():
    import svtav1_hip
    c = svtav1_hip.Context(0)
    yield c
    c.close()


def pictures(c, n):
    w, h, pics = bu.fixture_pictures(c)
    return w, h, pics[:n] if n > 1 else pics[1:2]     # one picture: the one with bits above bit 9


@pytest.mark.parametrize("c,n", CASES)
@pytest.mark.parametrize("with_n", (True, False))
def test_unpack(ctx, c, n, with_n):
    w, h, pics = pictures(c, n)
    src = bu.PlaneSet([p["in16"] for p in pics], np.uint16, seed=1)
    d8 = bu.PlaneSet(bu.blank_like([p["in16"] for p in pics], np.uint8), np.uint8, seed=2)
    dn = bu.PlaneSet(bu.blank_like([p["in16"] for p in pics], np.uint8), np.uint8, seed=0)
    ctx.pa_unpack_10bit_dev(src.upload(), src.planes(), d8.upload(), d8.planes(), dn.upload() if with_n else None, dn.planes(), w, h)
    ctx.synchronize()
    d8.check([p["out8"] for p in pics], "unpack, 8-bit planes")
    if with_n:
        dn.check([p["outn"] for p in pics], "unpack, 2-bit planes")


@pytest.mark.parametrize("c,n", CASES)
@pytest.mark.parametrize("compressed", (False, True))
def test_pack(ctx, c, n, compressed):
    w, h, pics = pictures(c, n)
    s8 = bu.PlaneSet([p["out8"] for p in pics], np.uint8, seed=1)
    sn = bu.TiledSet([p["tiled"] for p in pics]) if compressed else bu.PlaneSet([p["inn"] for p in pics], np.uint8, seed=2)
    dst = bu.PlaneSet(bu.blank_like([p["out8"] for p in pics], np.uint16), np.uint16, seed=0)
    ctx.pa_pack_10bit_dev(s8.upload(), s8.planes(), sn.upload(), sn.planes(), dst.upload(), dst.planes(), w, h, compressed=compressed)
    ctx.synchronize()
    dst.check([p["packc16" if compressed else "pack16"] for p in pics], "compressed pack" if compressed else "pack")


@pytest.mark.parametrize("c,n", CASES)
def test_picture_sse(ctx, c, n):
    """all five forms; the fixture holds what the reference leaves of the sums (truncated, Cb / Cr swapped), the restatement the sums"""
    import svtav1_hip
    w, h, pics = pictures(c, n)
    recon8 = bu.PlaneSet([p["recon8"] for p in pics], np.uint8, seed=1)
    recon16 = bu.PlaneSet([p["recon16"] for p in pics], np.uint16, seed=2)
    src8 = bu.PlaneSet([p["out8"] for p in pics], np.uint8, seed=0)
    srcn = bu.PlaneSet([p["inn"] for p in pics], np.uint8, seed=1)
    src16 = bu.PlaneSet([p["pack16"] for p in pics], np.uint16, seed=0)
    tiled = bu.TiledSet([p["tiled"] for p in pics])
    got = {"sse8": bu.device_sse(ctx, recon8, src8, w, h, len(pics)),
           "sse16": bu.device_sse(ctx, recon16, src16, w, h, len(pics), svtav1_hip.SSE_SRC_16BIT),
           "sse16_unpacked": bu.device_sse(ctx, recon16, src8, w, h, len(pics), svtav1_hip.SSE_SRC_UNPACKED, srcn),
           "sse16_compressed": bu.device_sse(ctx, recon16, src8, w, h, len(pics), svtav1_hip.SSE_SRC_COMPRESSED, tiled)}
    for j, p in enumerate(pics):
        want = bu.expected(p)
        for k in ("sse8", "sse16_unpacked", "sse16_compressed"):
            assert np.array_equal(bu.reference_fields(got[k][j]), p[k]), ((w, h), j, k)
            assert np.array_equal(got[k][j], want[k]), ((w, h), j, k)
        assert np.array_equal(got["sse16"][j], want["sse16_unpacked"]), ((w, h), j)


@pytest.mark.parametrize("c", range(len(bu.CASES)))
def test_maximal_differences_keep_64_bits(ctx, c):
    import svtav1_hip
    w, h, p = bu.fixture_max_difference(c)
    want = bu.expected_max_difference(p)
    recon8, recon16 = bu.PlaneSet([p["recon8"]], np.uint8), bu.PlaneSet([p["recon16"]], np.uint16)
    src8, srcn, tiled = bu.PlaneSet([p["in8"]], np.uint8, seed=1), bu.PlaneSet([p["inn"]], np.uint8, seed=2), bu.TiledSet([p["tiled"]])
    got = {"sse8": bu.device_sse(ctx, recon8, src8, w, h, 1),
           "sse16_unpacked": bu.device_sse(ctx, recon16, src8, w, h, 1, svtav1_hip.SSE_SRC_UNPACKED, srcn),
           "sse16_compressed": bu.device_sse(ctx, recon16, src8, w, h, 1, svtav1_hip.SSE_SRC_COMPRESSED, tiled)}
    for k in want:
        assert np.array_equal(got[k][0], want[k]), ((w, h), k)
        assert np.array_equal(bu.reference_fields(got[k][0]), p[k]), ((w, h), k)
    if c == 1:
        assert int(got["sse16_unpacked"][0][0]) >= 1 << 32


def test_unpack_over_a_padded_reference(ctx):
    """interior 72x40, borders 16 (chroma 8): width and height enlarged by the borders, the offsets those of the padded planes' first sample"""
    w, h, pics = bu.fixture_pictures(0)
    padded = [[bu.pad_edges(a, 16 if pl == 0 else 8) for pl, a in enumerate(p["in16"])] for p in pics[:2]]
    src = bu.PlaneSet(padded, np.uint16, seed=2)
    d8 = bu.PlaneSet(bu.blank_like(padded, np.uint8), np.uint8, seed=1)
    ctx.pa_unpack_10bit_dev(src.upload(), src.planes(), d8.upload(), d8.planes(), None, None, w + 32, h + 32)
    ctx.synchronize()
    d8.check([[bu.pad_edges(a, 16 if pl == 0 else 8) for pl, a in enumerate(p["out8"])] for p in pics[:2]], "unpack over a padded reference")


def test_validators_refuse_without_a_launch(ctx):
    """every refusal is SVTHIP_ERR_BAD_PARAMETER with a message; the destination is untouched afterwards"""
    import svtav1_hip
    w, h, pics = pictures(0, 1)
    src = bu.PlaneSet([pics[0]["in16"]], np.uint16)
    d8 = bu.PlaneSet(bu.blank_like([pics[0]["in16"]], np.uint8), np.uint8)
    d_src, d_d8 = src.upload(), d8.upload()
    import torch
    sse = torch.full((4,), -1, dtype=torch.int64, device="cuda:0")
    d_sse = sse.data_ptr()
    narrow = svtav1_hip.make_planes(d8.offsets[0], [w - 1, w // 2, w // 2])
    narrow_chroma = svtav1_hip.make_planes(d8.offsets[0], [w, w // 2, w // 2 - 1])
    negative = svtav1_hip.make_planes([-1, 0, 0], d8.strides[0])
    calls = {
        "width not a multiple of 8": lambda: ctx.pa_unpack_10bit_dev(d_src, src.planes(), d_d8, d8.planes(), None, None, w + 4, h),
        "height not a multiple of 8": lambda: ctx.pa_unpack_10bit_dev(d_src, src.planes(), d_d8, d8.planes(), None, None, w, h + 2),
        "width 0": lambda: ctx.pa_unpack_10bit_dev(d_src, src.planes(), d_d8, d8.planes(), None, None, 0, h),
        "null input": lambda: ctx.pa_unpack_10bit_dev(None, src.planes(), d_d8, d8.planes(), None, None, w, h),
        "null output": lambda: ctx.pa_unpack_10bit_dev(d_src, src.planes(), None, d8.planes(), None, None, w, h),
        "null 2-bit input": lambda: ctx.pa_pack_10bit_dev(d_d8, d8.planes(), None, d8.planes(), d_src, src.planes(), w, h),
        "null compressed input": lambda: ctx.pa_pack_10bit_dev(d_d8, d8.planes(), None, d8.planes(), d_src, src.planes(), w, h, compressed=True),
        "no pictures": lambda: ctx.pa_unpack_10bit_dev(d_src, [], d_d8, [], None, None, w, h),
        "too many pictures": lambda: ctx.pa_unpack_10bit_dev(d_src, src.planes() * 33, d_d8, d8.planes() * 33, None, None, w, h),
        "stride below the width": lambda: ctx.pa_unpack_10bit_dev(d_src, src.planes(), d_d8, [narrow], None, None, w, h),
        "chroma stride below the width": lambda: ctx.pa_pack_10bit_dev(d_d8, [narrow_chroma], d_d8, d8.planes(), d_src, src.planes(), w, h),
        "negative offset": lambda: ctx.pa_unpack_10bit_dev(d_src, src.planes(), d_d8, [negative], None, None, w, h),
        "odd 16-bit base": lambda: ctx.pa_unpack_10bit_dev(d_src + 1, src.planes(), d_d8, d8.planes(), None, None, w, h),
        "sse: null sums": lambda: ctx.picture_sse_dev(d_d8, d8.planes(), d_d8, d8.planes(), w, h, None),
        "sse: misaligned sums": lambda: ctx.picture_sse_dev(d_d8, d8.planes(), d_d8, d8.planes(), w, h, d_sse + 4),
        "sse: no pictures": lambda: ctx.picture_sse_dev(d_d8, [], d_d8, [], w, h, d_sse),
        "sse: unknown source form": lambda: ctx.highbd_picture_sse_dev(d_src, src.planes(), 3, d_d8, d8.planes(), d_d8, d8.planes(), w, h, d_sse),
        "sse: null 2-bit source": lambda: ctx.highbd_picture_sse_dev(d_src, src.planes(), svtav1_hip.SSE_SRC_UNPACKED, d_d8, d8.planes(), None, d8.planes(),
                                                                     w, h, d_sse),
        "sse: stride below the width": lambda: ctx.highbd_picture_sse_dev(d_src, src.planes(), svtav1_hip.SSE_SRC_16BIT, d_src, [narrow], None, None, w, h,
                                                                          d_sse),
    }
    for what, call in calls.items():
        with pytest.raises(svtav1_hip.SvtHipError) as e:
            call()
        code, _, message = str(e.value).partition(": ")
        assert BAD_PARAMETER in code and len(message) > 8, (what, str(e.value))
    ctx.synchronize()
    after = d8.download()
    assert (after[~d8.mask] == bu.GUARD).all() and not after[d8.mask].any() and (sse.cpu().numpy() == -1).all()
