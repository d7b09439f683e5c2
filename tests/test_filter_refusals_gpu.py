"""The order in which the three post-reconstruction filter families refuse a picture with two faults (deblocking, loop restoration,
CDEF): one entry of each family -- svthip_av1_[highbd_]loop_filter_sse_table_dev, svthip_av1_[highbd_]wiener_stats_dev,
svthip_av1_[highbd_]cdef_search_mse_dev -- and the two restoration entry bodies that take output planes.  Every case is refused on the
host before anything is launched; code and full text of svthip_last_error() are those of the library before the C-ABI glue was split by
family, which is the oracle here.  What that library does where one might expect otherwise:
  * the planes are checked plane by plane (null pointers, then strides, then alignment, of ONE plane before the next), so a null plane 1
    loses against a short stride of plane 0 and wins against a short stride of plane 1;
  * the sse-table entry looks at one plane only, so its two faults sit on the reconstruction and the source plane of that index;
  * a highbd entry checks its bit_depth argument (it must be 10) before it looks at the picture, so bit depth 9 is refused with that
    entry's text; "bit depth must be 8 or 10" is what svthip_cdef_pick_strengths_dev answers, which takes the bit depth as it comes."""
import pytest
import torch

import svtav1_hip

pytestmark = pytest.mark.gpu

W = H = 16
BAD = "svthip error 0x80001005: "
SIZE = "picture size must be a multiple of 8 each way, at most 16384 (got 12x16)"
NULL = "null pointer argument"
STRIDE0 = "stride of plane 0 is smaller than its width 16"
ALIGN = "16-bit planes must be 2-byte aligned"
BD10 = "bit_depth must be 10 (got 9)"
FULL, HALF = (W, W // 2, W // 2), (W // 2, W // 4, W // 4)   # strides that fit the planes; strides that do not


@pytest.fixture(scope="module")
def mem():
    """16x16 planes (room for 16-bit samples and an odd base) and the other arguments, all real device memory of the size a launch would
    need, though no case gets that far"""
    class Mem:
        pass
    m = Mem()
    plane = lambda: torch.zeros(W * H * 2 + 16, dtype=torch.uint8, device="cuda:0")  # noqa: E731
    m.keep = {k: [plane() for _ in range(3)] for k in ("recon", "deblocked", "source", "out")}
    m.recon, m.deblocked, m.source, m.out = ([t.data_ptr() for t in m.keep[k]] for k in ("recon", "deblocked", "source", "out"))
    m.work = torch.zeros(4 << 20, dtype=torch.uint8, device="cuda:0")
    assert svtav1_hip.lr_pick_workspace_bytes(W, H) <= m.work.numel()
    m.small = [torch.zeros(64 << 10, dtype=torch.uint8, device="cuda:0") for _ in range(6)]
    m.a, m.b, m.c, m.d, m.e, m.f = (t.data_ptr() for t in m.small)
    torch.cuda.synchronize()
    return m


def with_(seq, i, v):
    out = list(seq)
    out[i] = v
    return out


def refused(text, call, *args, **kw):
    with pytest.raises(svtav1_hip.SvtHipError) as e:
        call(*args, **kw)
    assert str(e.value) == BAD + text


# ---------------------------------------------------------------- the three picture checks

def lf_sse_table(ctx, m, bd=8, plane=0, width=W, recon=None, source=None, recon_stride=FULL, source_stride=FULL):
    pic = svtav1_hip.make_lf_picture(width, H, recon or m.recon, recon_stride, source or m.source, source_stride)
    ctx.av1_loop_filter_sse_table_dev(pic, m.a, W // 4, plane, 0, m.b, 0, m.c, bit_depth=bd)


def lr_stats(ctx, m, bd=8, ps=0, pe=3, width=W, cdef=None, deblocked=None, source=None, cdef_stride=FULL, deblocked_stride=FULL, source_stride=FULL):
    pic = svtav1_hip.make_lr_picture(width, H, cdef or m.recon, cdef_stride, deblocked or m.deblocked, deblocked_stride, source or m.source, source_stride)
    ctx.av1_wiener_stats_dev(pic, ps, pe, m.a, m.b, m.c, m.d, m.work.data_ptr(), bit_depth=bd)


def cdef_search_mse(ctx, m, bd=8, width=W, deblocked=None, source=None, deblocked_stride=FULL, source_stride=FULL):
    pic = svtav1_hip.make_cdef_picture(width, H, deblocked or m.deblocked, deblocked_stride, m.a, W // 4, source or m.source, source_stride)
    ctx.av1_cdef_search_mse_dev(pic, 100, m.b, m.c, bit_depth=bd)


ENTRIES = [lf_sse_table, lr_stats, cdef_search_mse]


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda f: f.__name__)
@pytest.mark.parametrize("bd", [8, 10])
def test_width_12_is_refused_with_the_size_message(hip_ctx, mem, entry, bd):
    refused(SIZE, entry, hip_ctx, mem, bd=bd, width=12)


def test_null_plane_wins_over_a_short_stride_of_the_same_plane_index(hip_ctx, mem):
    m = mem
    refused(NULL, lf_sse_table, hip_ctx, m, plane=1, recon=with_(m.recon, 1, None), source_stride=with_(FULL, 1, 4))
    refused(NULL, lr_stats, hip_ctx, m, deblocked=with_(m.deblocked, 1, None), cdef_stride=with_(FULL, 1, 4))
    refused(NULL, lr_stats, hip_ctx, m, source=with_(m.source, 1, None), cdef_stride=with_(FULL, 1, 4))
    refused(NULL, cdef_search_mse, hip_ctx, m, source=with_(m.source, 1, None), deblocked_stride=with_(FULL, 1, 4))


def test_short_stride_of_an_earlier_plane_wins_over_a_null_plane(hip_ctx, mem):
    m = mem
    refused(STRIDE0, lr_stats, hip_ctx, m, deblocked=with_(m.deblocked, 1, None), cdef_stride=HALF)
    refused(STRIDE0, cdef_search_mse, hip_ctx, m, deblocked=with_(m.deblocked, 1, None), deblocked_stride=HALF)
    # and the other way round: a null plane 0 before the short stride of plane 1
    refused(NULL, lr_stats, hip_ctx, m, cdef=with_(m.recon, 0, None), deblocked_stride=with_(FULL, 1, 4))
    refused(NULL, cdef_search_mse, hip_ctx, m, deblocked=with_(m.deblocked, 0, None), source_stride=with_(FULL, 1, 4))


def test_short_stride_wins_over_an_odd_16_bit_plane_address(hip_ctx, mem):
    m = mem
    refused(STRIDE0, lf_sse_table, hip_ctx, m, bd=10, recon=with_(m.recon, 0, m.recon[0] + 1), source_stride=HALF)
    refused(STRIDE0, lr_stats, hip_ctx, m, bd=10, cdef=with_(m.recon, 0, m.recon[0] + 1), deblocked_stride=HALF)
    refused(STRIDE0, lr_stats, hip_ctx, m, bd=10, deblocked=with_(m.deblocked, 0, m.deblocked[0] + 1), source_stride=HALF)
    refused(STRIDE0, cdef_search_mse, hip_ctx, m, bd=10, deblocked=with_(m.deblocked, 0, m.deblocked[0] + 1), source_stride=HALF)


def test_odd_16_bit_plane_address_alone(hip_ctx, mem):
    m = mem
    refused(ALIGN, lf_sse_table, hip_ctx, m, bd=10, source=with_(m.source, 0, m.source[0] + 1))
    refused(ALIGN, lr_stats, hip_ctx, m, bd=10, source=with_(m.source, 2, m.source[2] + 1))
    refused(ALIGN, cdef_search_mse, hip_ctx, m, bd=10, deblocked=with_(m.deblocked, 1, m.deblocked[1] + 1))
    refused("stride of plane 2 is smaller than its width 8", lr_stats, hip_ctx, m, source_stride=with_(FULL, 2, 7))


def test_bit_depth_9_wins_over_width_12(hip_ctx, mem):
    refused(BD10, lr_stats, hip_ctx, mem, bd=9, width=12)
    refused(BD10, cdef_search_mse, hip_ctx, mem, bd=9, width=12)
    # the pick takes the bit depth as it comes; no filter block is its second fault
    refused("bit depth must be 8 or 10 (got 9)", hip_ctx.cdef_pick_strengths_dev, mem.a, mem.b, 0, 0, 100, 9, mem.c, mem.d)


def test_restoration_empty_plane_range_wins_over_width_12(hip_ctx, mem):
    refused("planes [1, 1) are empty or not within 0..3", lr_stats, hip_ctx, mem, ps=1, pe=1, width=12)
    refused("planes [1, 1) are empty or not within 0..3", lr_stats, hip_ctx, mem, bd=10, ps=1, pe=1, width=12)


# ---------------------------------------------------------------- the restoration entries with output planes

def lr_filter_frame(ctx, m, bd=8, out=None, out_stride=FULL):
    pic = svtav1_hip.make_lr_picture(W, H, m.recon, FULL, m.deblocked, FULL)
    ctx.av1_lr_filter_frame_dev(pic, out or m.out, out_stride, 0, 3, m.a, m.b, m.c, bit_depth=bd)


def lr_pick_filter(ctx, m, bd=8, out=None, out_stride=FULL):
    pic = svtav1_hip.make_lr_picture(W, H, m.recon, FULL, m.deblocked, FULL, m.source, FULL)
    ctx.av1_pick_filter_restoration_dev(pic, (1000, (1, 2), (3, 4), (5, 6, 7)), m.work.data_ptr(), out or m.out, out_stride, m.a, m.b, m.c, m.d, bit_depth=bd)


@pytest.mark.parametrize("entry", [lr_filter_frame, lr_pick_filter], ids=lambda f: f.__name__)
def test_restoration_output_planes(hip_ctx, mem, entry):
    m = mem
    short = "output stride of plane 2 is smaller than its width"
    refused(NULL, entry, hip_ctx, m, out=with_(m.out, 1, None))
    refused(short, entry, hip_ctx, m, out_stride=with_(FULL, 2, 4))
    refused(NULL, entry, hip_ctx, m, out=with_(m.out, 1, None), out_stride=with_(FULL, 2, 4))
    refused(short, entry, hip_ctx, m, bd=10, out=with_(m.out, 2, m.out[2] + 1), out_stride=with_(FULL, 2, 4))
    refused(ALIGN, entry, hip_ctx, m, bd=10, out=with_(m.out, 2, m.out[2] + 1))
