"""GPU: mode decision's partition decision (svthip_md_partition_batch_dev, _compose_dev, _picture_dev) through the C ABI, bit-exact against
the restatement (tests/md_part_util.py: expected() computes a case once and is shared; tests/test_md_part_vs_ref.py holds it to the
fixture and the reference) for every per-block record, final list, count and composed plane of every case.  The pool and the destination
sit inside guarded garbage.  Every case runs in two layouts of tests/test_md_full_gpu.py's _Planes: a multiple-of-4 base and stride (2056 /
1032 for the pool, 144 / 76 or 272 / 140 for the picture: rows move in units of 8 and 4 bytes at most) and 3 bytes into the buffer at an odd
stride (single bytes).  The 16-byte unit, the one pictures with strides that are multiples of 16 take, has cases of its own
(test_strides_of_16_take_the_widest_unit: _Planes16, all three planes compared, the columns between width and stride guarded).  The
outputs are pre-filled, so a write behind a row, a list or a plane shows."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import md_part_util as pu  # noqa: E402
import svtav1_hip  # noqa: E402
from test_md_full_gpu import GUARD, _dev, _Planes  # noqa: E402

pytestmark = pytest.mark.gpu

BAD = "80001005"


class _Planes16:
    """Y, Cb, Cr on the device at a 256-byte aligned base and a stride that is a multiple of 16 whatever the width (width rounded up to 16,
    plus 16), a guard row above and below and guard columns behind every row; the interface of _Planes"""

    def __init__(self, torch, planes):
        self.shapes, self.host, self.dev, self.strides = [p.shape for p in planes], [], [], []
        for k, p in enumerate(planes):
            h, w = p.shape
            stride = (planes[min(k, 1)].shape[1] + 15) // 16 * 16 + 16
            buf = np.full((h + 2, stride), 0x3C, np.uint8)
            buf[1:1 + h, :w] = p
            self.host.append(buf)
            self.dev.append(_dev(torch, buf))
            self.strides.append(stride)
            assert self.dev[-1].data_ptr() % 256 == 0 and stride % 16 == 0
        self.arg = svtav1_hip.InterPlanes()
        self.arg.y, self.arg.cb, self.arg.cr = (t.data_ptr() + st for t, st in zip(self.dev, self.strides))
        self.arg.y_stride, self.arg.c_stride = self.strides[0], self.strides[1]

    def download(self):
        """the planes; asserts that nothing around them changed"""
        out = []
        for buf, t, (h, w) in zip(self.host, self.dev, self.shapes):
            got = t.cpu().numpy().reshape(buf.shape)
            out.append(got[1:1 + h, :w].copy())
            rest = got.copy()
            rest[1:1 + h, :w] = buf[1:1 + h, :w]
            assert np.array_equal(rest, buf), "wrote outside a plane"
        return out


class _Call:
    """one scenario on the device: its arrays, planes and pre-filled outputs; shift None puts the planes at strides that are multiples of 16"""

    def __init__(self, torch, ctx, s, shift, sbs=None, leaves=None, decisions=None):
        self.torch, self.ctx, self.s = torch, ctx, s
        self.sbs, self.leaves, self.decisions = (s.sbs if sbs is None else sbs), (s.leaves if leaves is None else leaves), \
            (s.decisions if decisions is None else decisions)
        self.n_sb, self.n, self.max_final = len(self.sbs), len(pu.geometry(s.sb_size)), 1024 if s.sb_size == 128 else 256
        dst0 = [np.full((s.h, s.w), 0xA5, np.uint8), *(np.full(((s.h + 1) // 2, (s.w + 1) // 2), 0xA5, np.uint8) for _ in range(2))]
        self.pool, self.dst = (_Planes16(torch, s.pool), _Planes16(torch, dst0)) if shift is None else (_Planes(torch, s.pool, shift), _Planes(torch, dst0, shift))
        self.d_sb, self.d_leaf, self.d_decision = _dev(torch, self.sbs), _dev(torch, self.leaves), _dev(torch, self.decisions)
        full = lambda n: torch.full((n,), GUARD, dtype=torch.uint8, device="cuda:0")  # noqa: E731
        self.d_result, self.d_final, self.d_count = full((self.n_sb * self.n + 1) * 16), full((self.n_sb * self.max_final + 1) * 16), full((self.n_sb + 1) * 4)
        torch.cuda.synchronize()

    def decide_args(self):
        s = self.s
        return dict(d_sb=self.d_sb.data_ptr(), n_sb=self.n_sb, d_leaf=self.d_leaf.data_ptr(), n_leaf=len(self.leaves), d_decision=self.d_decision.data_ptr(),
                    n_decision=len(self.decisions), sb_size=s.sb_size, slice_is_intra=int(s.intra), partition_fac_bits=s.fac,
                    d_result=self.d_result.data_ptr(), d_final=self.d_final.data_ptr(), d_final_count=self.d_count.data_ptr())

    def compose_args(self, **kw):
        s = self.s
        return dict(dict(pool=self.pool.arg, pool_width=s.pool_w, pool_height=s.pool_h, dst=self.dst.arg, width=s.w, height=s.h), **kw)

    def decide(self, stream=None):
        self.ctx.md_partition_batch_dev(**self.decide_args(), stream=stream)

    def compose(self, stream=None, **kw):
        self.ctx.md_partition_compose_dev(n_sb=self.n_sb, d_leaf=self.d_leaf.data_ptr(), n_leaf=len(self.leaves), sb_size=self.s.sb_size,
                                          d_final=self.d_final.data_ptr(), d_final_count=self.d_count.data_ptr(), **self.compose_args(**kw), stream=stream)

    def picture(self, stream=None):
        self.ctx.md_partition_picture_dev(**self.decide_args(), **self.compose_args(), stream=stream)

    def finish(self):
        """(result rows, final rows, counts, destination planes) after a synchronisation; the guards are checked"""
        self.ctx.synchronize()
        self.torch.cuda.synchronize()
        raw_r, raw_f, raw_c = self.d_result.cpu().numpy(), self.d_final.cpu().numpy(), self.d_count.cpu().numpy()
        assert (raw_r[-16:] == GUARD).all() and (raw_f[-16:] == GUARD).all() and (raw_c[-4:] == GUARD).all(), "wrote behind the last row"
        return (raw_r[:-16].view(pu.RESULT_DTYPE).reshape(self.n_sb, self.n), raw_f[:-16].view(pu.FINAL_DTYPE).reshape(self.n_sb, self.max_final),
                raw_c[:-4].view(np.uint32), self.dst.download())


def _check(got, e, what, planes=True):
    result, final, count, dst = got
    assert np.array_equal(count, e["count"]), (what, count, e["count"])
    for k in range(len(count)):
        assert np.array_equal(result[k], e["result"][k]), (what, "result of superblock", k, np.nonzero(result[k] != e["result"][k])[0][:5])
        assert np.array_equal(final[k][:count[k]], e["final"][k][:count[k]]), (what, "final list of superblock", k)
        assert (final[k][count[k]:].view(np.uint8) == GUARD).all(), (what, "wrote behind the final list of superblock", k)
    if planes:
        for p, (a, b) in enumerate(zip(dst, e["dst"])):
            assert np.array_equal(a, b), (what, "composed plane", p, np.argwhere(a != b)[:4])


def _refused(ctx, n):
    if n == 0:
        assert ctx.inter_pred_refused() == 0
        return
    with pytest.raises(svtav1_hip.SvtHipError, match=rf"{BAD}: {n} PU\(s\) or unit\(s\) refused"):
        ctx.inter_pred_refused()
    assert ctx.inter_pred_refused() == 0


@pytest.mark.parametrize("name", pu.CASES)
def test_every_case_bit_exact(hip_ctx, name):
    """both pictures, the four lists, intra and inter, the cost variants, the irregular list and the final block without a leaf (counted):
    the decision and the composition as two calls, then svthip_md_partition_picture_dev on another stream with the planes at an odd offset"""
    torch = pytest.importorskip("torch")
    s, e = pu.scenario(name), pu.expected(name)
    hip_ctx.inter_pred_refused()
    call = _Call(torch, hip_ctx, s, 0)
    call.decide()
    call.compose()
    _check(call.finish(), e, (name, "two calls"))
    _refused(hip_ctx, e["refused"])
    call = _Call(torch, hip_ctx, s, 3)
    stream = torch.cuda.Stream()
    call.picture(stream=stream.cuda_stream)
    stream.synchronize()
    _check(call.finish(), e, (name, "one call"))
    _refused(hip_ctx, e["refused"])


@pytest.mark.parametrize("name", ("p64-all-p-v0", "p128-all-p-v1", "p128-sq-i-v0"))
def test_strides_of_16_take_the_widest_unit(hip_ctx, name):
    """pool and picture at 256-byte aligned bases and strides that are multiples of 16: every tile at a 16-aligned position whose width
    allows it moves in 16-byte units, in Y, Cb and Cr (the case must hold such tiles in all three: counted here from the rule); all
    three planes and the guard columns behind their rows are compared; the two-call and the one-call form"""
    torch = pytest.importorskip("torch")
    s, e = pu.scenario(name), pu.expected(name)
    wide = [0, 0]
    for k in range(len(s.origins)):
        for f in e["final"][k][:e["count"][k]]:
            leaf = s.leaves[int(f["leaf"])]
            x, px, w = int(f["x"]), int(leaf["pool_x"]), int(f["bwidth"])
            wide[0] += (x | px | w) % 16 == 0
            wide[1] += bool(f["has_uv"]) and (((x >> 3) << 3) // 2 | ((px >> 3) << 3) // 2 | w // 2) % 16 == 0
    assert wide[0] >= 2 and wide[1] >= 2, wide
    hip_ctx.inter_pred_refused()
    call = _Call(torch, hip_ctx, s, None)
    call.decide()
    call.compose()
    _check(call.finish(), e, (name, "two calls, strides of 16"))
    call = _Call(torch, hip_ctx, s, None)
    call.picture()
    _check(call.finish(), e, (name, "one call, strides of 16"))
    _refused(hip_ctx, 0)


def _start_state(sb_size):
    g = pu.geometry(sb_size)
    r = np.zeros(len(g), pu.RESULT_DTYPE)
    r["cost"], r["leaf"] = pu.MAX_MODE_COST, pu.NONE
    r["part"], r["flags"] = np.where(g["shape"] == 0, pu.SPLIT, 0), np.where(g["shape"] == 0, 1, 0)
    return r


def test_lists_refused_on_the_device(hip_ctx):
    """an mds_idx beyond the table, an mds_idx not above its predecessor's, a decision_index beyond n_decision, a leaf_count above the
    block count (its range inside n_leaf) and a leaf range beyond n_leaf, one count each: the superblock keeps the start state and gets no
    final block, the other is decided as before"""
    torch = pytest.importorskip("torch")
    name = "p64-sq-p-v0"
    s, e = pu.scenario(name), pu.expected(name)
    leaves, sbs = np.concatenate([s.leaves, np.zeros(1200, pu.LEAF_DTYPE)]), s.sbs.copy()   # room behind the lists: 1102 leaves fit in n_leaf
    first = sbs["first_leaf"].tolist()
    sbs["leaf_count"][3] = 1102                                              # superblock 3: more leaves than blocks
    leaves["mds_idx"][first[1] - 1] = 1101                                   # superblock 0: its last leaf is beyond the table
    leaves["mds_idx"][first[1] + 3] = leaves["mds_idx"][first[1] + 2]        # superblock 1: not ascending
    leaves["decision_index"][first[2]] = len(s.decisions)                    # superblock 2: beyond n_decision
    sbs["leaf_count"][5] = len(leaves) - first[5] + 1                        # superblock 5: its range passes n_leaf
    hip_ctx.inter_pred_refused()
    call = _Call(torch, hip_ctx, s, 0, sbs=sbs, leaves=leaves)
    call.picture()
    result, final, count, dst = call.finish()
    _refused(hip_ctx, 5)
    want_dst = [np.full(p.shape, 0xA5, np.uint8) for p in e["dst"]]
    for k in range(6):
        if k == 4:
            assert count[k] == e["count"][k] and np.array_equal(result[k], e["result"][k]) and np.array_equal(final[k][:count[k]], e["final"][k][:count[k]])
            for f in e["final"][k][:count[k]]:
                pu.compose_block(want_dst, s.pool, f, s.leaves[int(f["leaf"])])
        else:
            assert count[k] == 0 and np.array_equal(result[k], _start_state(64)), k
            assert (final[k].view(np.uint8) == GUARD).all()
    assert all(np.array_equal(a, b) for a, b in zip(dst, want_dst))


def test_tiles_outside_a_plane_are_skipped_and_counted(hip_ctx):
    """the composition with a picture and a pool stated smaller than the lists need: the blocks that no longer fit are counted and nothing
    of them is copied, the others land as before; the guards around the planes are unchanged (download() asserts it)"""
    torch = pytest.importorskip("torch")
    name = "p64-all-p-v0"
    s, e = pu.scenario(name), pu.expected(name)
    hip_ctx.inter_pred_refused()
    call = _Call(torch, hip_ctx, s, 0)
    call.decide()
    call.compose(width=s.w - 8, height=s.h - 8)
    result, final, count, dst = call.finish()
    want = [np.full(p.shape, 0xA5, np.uint8) for p in e["dst"]]
    skipped = 0
    for k in range(len(count)):
        for f in e["final"][k][:count[k]]:
            if int(f["x"]) + int(f["bwidth"]) > s.w - 8 or int(f["y"]) + int(f["bheight"]) > s.h - 8:
                skipped += 1
            else:
                pu.compose_block(want, s.pool, f, s.leaves[int(f["leaf"])])
    assert skipped > 0 and all(np.array_equal(a, b) for a, b in zip(dst, want))
    _refused(hip_ctx, skipped)
    _check((result, final, count, dst), e, name, planes=False)


def test_final_lists_the_composition_refuses(hip_ctx):
    """svthip_md_partition_compose_dev on final lists a caller spoiled: a count above max_final (the superblock is counted once and nothing
    of it is copied), a record whose leaf is beyond n_leaf but not SVTHIP_MD_PART_NONE (counted, skipped), a record without a leaf
    (skipped, not counted again: the decision counted it)"""
    torch = pytest.importorskip("torch")
    name = "p64-sq-p-v0"
    s, e = pu.scenario(name), pu.expected(name)
    final, count = e["final"].copy(), e["count"].copy()
    count[0] = 257
    final[1][0]["leaf"] = len(s.leaves)
    final[2][1]["leaf"] = pu.NONE
    hip_ctx.inter_pred_refused()
    call = _Call(torch, hip_ctx, s, 0)
    d_final, d_count = _dev(torch, final), _dev(torch, count)
    torch.cuda.synchronize()
    hip_ctx.md_partition_compose_dev(n_sb=len(count), d_leaf=call.d_leaf.data_ptr(), n_leaf=len(s.leaves), sb_size=64, d_final=d_final.data_ptr(),
                                     d_final_count=d_count.data_ptr(), **call.compose_args())
    hip_ctx.synchronize()
    _refused(hip_ctx, 2)
    want = [np.full(p.shape, 0xA5, np.uint8) for p in e["dst"]]
    for k in range(1, len(count)):
        for j, f in enumerate(e["final"][k][:count[k]]):
            if (k, j) not in ((1, 0), (2, 1)):
                pu.compose_block(want, s.pool, f, s.leaves[int(f["leaf"])])
    got = call.dst.download()
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and not all(np.array_equal(a, b) for a, b in zip(got, e["dst"]))


def test_no_superblocks_is_ok(hip_ctx):
    torch = pytest.importorskip("torch")
    s = pu.scenario("p64-sq-p-v0")
    call = _Call(torch, hip_ctx, s, 0)
    hip_ctx.md_partition_batch_dev(**dict(call.decide_args(), n_sb=0))
    hip_ctx.md_partition_picture_dev(**dict(call.decide_args(), n_sb=0), **call.compose_args())
    hip_ctx.synchronize()
    assert (call.d_result.cpu().numpy() == GUARD).all() and (call.d_count.cpu().numpy() == GUARD).all()
