"""numpy restatement of the 10-bit picture forms (svthip_pa_unpack_10bit_dev, svthip_pa_pack_10bit_dev, svthip_pa_pack_10bit_compressed_dev,
svthip_picture_sse_dev, svthip_highbd_picture_sse_dev), written from the reference's C:
  EB_ENC_msbUnPack2D / UnPack8BitData / EB_ENC_msbPack2D / CompressedPackmsb   Source/Lib/C_DEFAULT/EbPackUnPack_C.c:127-174, :12-86
  the SB-tiled compressed 2-bit plane as CompressedPackLcu is handed it         Source/Lib/Codec/EbCodingLoop.c:2888-2929
  PsnrCalculations                                                              Source/Lib/Codec/EbEncDecProcess.c:775-1133
Also the fixture's access (tests/golden/bitdepth.npz, written by tests/golden/make_golden_bitdepth.py), the constructed pictures the fixture
holds, plane sets with offsets and strides that are no multiples of 16 bytes and guard bytes around every row, and the device round trips."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bitdepth.npz")
CASES = ((72, 40), (136, 72))    # luma width, height
N_PICS = 3                       # pictures per case
PLANES = ("y", "cb", "cr")
GUARD = 0xA5
MD_PIC, MD_BORDER = (72, 40), 40  # the 10-bit references of the mode-decision prediction cases: interior, luma border
MD_UNDEFINED_NOTE = """AV1InterPrediction10BitMD copies every block it filters into a local 8-bit buffer first (Av1UnPackReferenceBlock ->
extract8_bitdata_safe_sub, which is EB_ENC_UnPack8BitDataSafeSub_SSE2_INTRIN for every asm_type, ASM_SSE2/EbPackUnPack_Intrinsic_SSE2.c:412-767).
For the sub-8x8 chroma pieces of a block 4 wide the copied width is 2 + 8 = 10; the copy's last branch (:736-761) walks a row in steps of
four, twelve columns, but rewinds by the width, ten, so every pair of rows lands two columns further right in the source AND in the local
buffer.  The samples sit where they belong, but from the third row on the leftmost columns the filter reads were never written: the
prediction of Cb and Cr then depends on what an earlier call left in the buffer.  A width of 12 (blocks 4 high: 8x4, 16x4) is walked
correctly.  So the reference has no defined chroma output for a 4-wide block with sub-8x8 chroma; there the restatement -- the 8-bit
prediction from the >> 2 references, which is what the function computes wherever it is defined -- is the only pin."""
MD_CHROMA_UNDEFINED = ("uni_4x8_sub8x8_chroma",)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement

def unpack(in16):
    """EB_ENC_msbUnPack2D: (uint8_t)(in >> 2), (uint8_t)(in << 6); the casts decide what bits above bit 9 do"""
    a = np.asarray(in16, np.uint16).astype(np.uint32)
    return ((a >> 2) & 0xff).astype(np.uint8), ((a << 6) & 0xff).astype(np.uint8)


def pack(in8, inn):
    """EB_ENC_msbPack2D: (in8 << 2) | ((inn >> 6) & 3)"""
    return ((np.asarray(in8, np.uint8).astype(np.uint16) << 2) | ((np.asarray(inn, np.uint8).astype(np.uint16) >> 6) & 3)).astype(np.uint16)


def sb_size(plane):
    return 64 if plane == 0 else 32


def _sbs(pw, ph, sb):
    for sb_y in range(0, ph, sb):
        for sb_x in range(0, pw, sb):
            yield sb_x, sb_y, min(sb, pw - sb_x), min(sb, ph - sb_y)


def to_tiled(inn, sb):
    """The reference's compressed plane of an unpacked 2-bit plane (bits 7..6 of every byte): four samples a byte, the first in bits 7..6;
    the SBs in raster order, each sb_h rows of sb_w / 4 bytes, at sb_y * (pw / 4) + (sb_x / 4) * sb_h."""
    ph, pw = inn.shape
    two = (np.asarray(inn, np.uint8) >> 6).astype(np.uint8)
    four = ((two[:, 0::4] << 6) | (two[:, 1::4] << 4) | (two[:, 2::4] << 2) | two[:, 3::4]).astype(np.uint8)
    out = np.zeros(pw * ph // 4, np.uint8)
    for sb_x, sb_y, sb_w, sb_h in _sbs(pw, ph, sb):
        at = sb_y * (pw // 4) + (sb_x // 4) * sb_h
        out[at:at + sb_h * (sb_w // 4)] = four[sb_y:sb_y + sb_h, sb_x // 4:(sb_x + sb_w) // 4].reshape(-1)
    return out


def from_tiled(tiled, pw, ph, sb):
    """The unpacked 2-bit plane (low six bits zero) of a compressed plane"""
    four = np.zeros((ph, pw // 4), np.uint8)
    for sb_x, sb_y, sb_w, sb_h in _sbs(pw, ph, sb):
        at = sb_y * (pw // 4) + (sb_x // 4) * sb_h
        four[sb_y:sb_y + sb_h, sb_x // 4:(sb_x + sb_w) // 4] = np.asarray(tiled[at:at + sb_h * (sb_w // 4)], np.uint8).reshape(sb_h, sb_w // 4)
    out = np.zeros((ph, pw), np.uint8)
    for i in range(4):
        out[:, i::4] = ((four >> (6 - 2 * i)) & 3) << 6
    return out


def pack_compressed(in8, tiled, sb):
    """CompressedPackmsb over every SB of a plane"""
    ph, pw = in8.shape
    return pack(in8, from_tiled(tiled, pw, ph, sb))


def sse(a, b):
    """one plane's sum of squared differences, the full 64-bit number"""
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return np.uint64(int((d * d).sum()))


def picture_sse(recon, src):
    """[3] uint64 in plane order Y, Cb, Cr"""
    return np.array([sse(r, s) for r, s in zip(recon, src)], np.uint64)


def reference_fields(sums):
    """What PsnrCalculations leaves of the sums in (luma_sse, cb_sse, cr_sse): each truncated to uint32_t, the Cb sum in cr_sse and the Cr
    sum in cb_sse (:858-860, :1129-1131)"""
    t = (np.asarray(sums, np.uint64) & np.uint64(0xffffffff)).astype(np.uint32)
    return np.array([t[0], t[2], t[1]], np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fixture and its pictures

def plane_dims(w, h):
    return ((h, w), (h // 2, w // 2), (h // 2, w // 2))


def make_pictures(rng, w, h):
    """N_PICS constructed pictures of a case, each a dict of plane lists:
      in16   the 16-bit input.  Picture 0 is clean 10-bit video (ramps plus noise); picture 1 has random bits above bit 9 set in a third of
             its samples; picture 2 is wholly random 16-bit words
      inn    an unpacked 2-bit plane whose low six bits are NOT zero (random bytes), to be packed with in8 = in16 >> 2
      tiled  a compressed plane of random bytes
      recon8 / recon16   reconstructions: the source plus an error of a few steps, clipped; picture 2's recon16 is random 16-bit words"""
    pics = []
    for i in range(N_PICS):
        p = {k: [] for k in ("in16", "inn", "tiled", "recon8", "recon16")}
        for c, (ph, pw) in enumerate(plane_dims(w, h)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            a = ((xx * (9 + 2 * c) + yy * (5 + i) + (xx * yy >> 3)) % 1024 + rng.integers(-12, 13, (ph, pw))).clip(0, 1023).astype(np.uint16)
            if i == 1:
                a = np.where(rng.random((ph, pw)) < 1 / 3, a | (rng.integers(1, 64, (ph, pw)) << 10), a).astype(np.uint16)
            if i == 2:
                a = rng.integers(0, 65536, (ph, pw)).astype(np.uint16)
            a[0, 0], a[-1, -1] = 0xffff, 0x03ff
            p["in16"].append(a)
            p["inn"].append(rng.integers(0, 256, (ph, pw)).astype(np.uint8))
            p["tiled"].append(rng.integers(0, 256, pw * ph // 4).astype(np.uint8))
            in8 = unpack(a)[0]
            p["recon8"].append((in8.astype(np.int32) + rng.integers(-9, 10, (ph, pw))).clip(0, 255).astype(np.uint8))
            r16 = (pack(in8, p["inn"][-1]).astype(np.int32) + rng.integers(-30, 31, (ph, pw))).clip(0, 1023).astype(np.uint16)
            p["recon16"].append(rng.integers(0, 65536, (ph, pw)).astype(np.uint16) if i == 2 else r16)
        pics.append(p)
    return pics


def max_difference_picture(w, h, rng):
    """0 against the largest sample everywhere: the 8-bit source all zero, the 2-bit bytes with nothing but their ignored low six bits set,
    the compressed bytes zero; the reconstructions 255 and 1023.  Sums: 255^2 and 1023^2 times the samples of the plane."""
    p = {k: [] for k in ("in8", "inn", "tiled", "recon8", "recon16")}
    for ph, pw in plane_dims(w, h):
        p["in8"].append(np.zeros((ph, pw), np.uint8))
        p["inn"].append(rng.integers(0, 64, (ph, pw)).astype(np.uint8))
        p["tiled"].append(np.zeros(pw * ph // 4, np.uint8))
        p["recon8"].append(np.full((ph, pw), 255, np.uint8))
        p["recon16"].append(np.full((ph, pw), 1023, np.uint16))
    return p


def expected(p):
    """Everything the entries make of one picture of make_pictures, by the restatement"""
    e = {k: [] for k in ("out8", "outn", "pack16", "packc16")}
    for c in range(3):
        o8, on = unpack(p["in16"][c])
        e["out8"].append(o8), e["outn"].append(on)
        e["pack16"].append(pack(o8, p["inn"][c]))
        e["packc16"].append(pack_compressed(o8, p["tiled"][c], sb_size(c)))
    e["sse8"] = picture_sse(p["recon8"], e["out8"])
    e["sse16_unpacked"] = picture_sse(p["recon16"], e["pack16"])
    e["sse16_compressed"] = picture_sse(p["recon16"], e["packc16"])
    return e


def expected_max_difference(p):
    n = np.array([a.size for a in p["in8"]], np.uint64)
    return {"sse8": n * np.uint64(255 * 255), "sse16_unpacked": n * np.uint64(1023 * 1023), "sse16_compressed": n * np.uint64(1023 * 1023)}


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = dict(np.load(FIXTURE))
    return _fixture


def fixture_pictures(c):
    """(w, h, [picture dicts]) of case c: the inputs of make_pictures and the reference's outputs under the keys of expected(); the
    SSE entries are the reference's three fields (reference_fields), not the sums"""
    z = fixture()
    w, h = (int(v) for v in z["case"][c])
    pics = []
    for i in range(N_PICS):
        p = {}
        for k in ("in16", "inn", "tiled", "recon8", "recon16", "out8", "outn", "pack16", "packc16"):
            p[k] = [z[f"c{c}_p{i}_{k}_{pl}"] for pl in PLANES]
        for k in ("sse8", "sse16_unpacked", "sse16_compressed"):
            p[k] = z[f"c{c}_p{i}_{k}"]
        pics.append(p)
    return w, h, pics


def fixture_max_difference(c):
    z = fixture()
    w, h = (int(v) for v in z["case"][c])
    p = {k: [z[f"c{c}_max_{k}_{pl}"] for pl in PLANES] for k in ("in8", "inn", "tiled", "recon8", "recon16")}
    for k in ("sse8", "sse16_unpacked", "sse16_compressed"):
        p[k] = z[f"c{c}_max_{k}"]
    return w, h, p


# ---------------------------------------------------------------------------------------------------------------------------------------
# the 10-bit references of the mode-decision prediction cases

def md_reference_interiors():
    """Two 10-bit pictures of MD_PIC samples without borders, integer arithmetic only: ramps, a hash texture in the low two bits (so that
    >> 2 loses something), saturated and zero stripes.  [(y, cb, cr)] * 2"""
    w, h = MD_PIC
    out = []
    for t in range(2):
        planes = []
        for k, (ph, pw) in enumerate(plane_dims(w, h)):
            yy, xx = np.mgrid[0:ph, 0:pw].astype(np.int64)
            ramp = (xx * (23 + 6 * t + 2 * k) + yy * (13 + 3 * t) + (xx * yy >> (2 + k))) % 2046
            tri = np.where(ramp <= 1023, ramp, 2046 - ramp)
            hsh = (xx * 0x9E3779B1 + yy * 0x85EBCA77 + (3 * t + k + 1) * 0xC2B2AE3D) & 0xFFFFFFFF
            hsh = ((hsh ^ (hsh >> 15)) * 0x2C1B3C6D) & 0xFFFFFFFF
            a = (tri & ~3) | ((hsh >> 13) & 3)
            a[(yy // 9 + xx // 13) % 11 == 0] = 1023
            a[(yy // 7 + xx // 5) % 13 == 0] = 0
            planes.append(a.astype(np.uint16))
        out.append(tuple(planes))
    return out


def pad_edges(plane, border):
    """generate_padding / generate_padding16_bit: the edge samples replicated"""
    return np.pad(plane, border, mode="edge")


def md_cases():
    """[(name, bw, bh, desc)]: a uni-predicted 8x8, a bi-predicted 16x16, a uni-predicted 4x8 that carries sub-8x8 chroma (its left neighbour
    inter, on list 1), and an 8x8 whose vector is clamped far inside the border.  One PU each; the descriptors are those of
    svthip_av1_inter_pred_batch_dev."""
    import inter_pred_util as ipu
    import svtav1_hip
    w, h = MD_PIC

    def desc(bw, bh, x, y, direction, mv0, mv1, filters):
        d = np.zeros(1, svtav1_hip.INTER_PU_DESC_DTYPE)
        d["pu_origin_x"], d["pu_origin_y"], d["dst_origin_x"], d["dst_origin_y"] = x, y, x, y
        d["mb_to_left_edge"], d["mb_to_right_edge"] = -x * 8, (w - bw - x) * 8
        d["mb_to_top_edge"], d["mb_to_bottom_edge"] = -y * 8, (h - bh - y) * 8
        d["interp_filters"], d["pred_direction"], d["own_list"] = filters, direction, int(direction == 1)
        d["has_uv"] = ipu.geometry_has_uv(bw, bh, x, y)
        d["mv"][0] = (mv0, mv1)
        return d

    uni8 = desc(8, 8, 24, 16, 0, (13, -22), (0, 0), (1 << 16) | 0)
    bi16 = desc(16, 16, 48, 16, 2, (-37, 9), (20, 45), (0 << 16) | 2)
    sub8 = desc(4, 8, 12, 8, 0, (7, 18), (0, 0), (2 << 16) | 1)
    sub8["nb_is_inter"][0][2], sub8["nb_list"][0][2], sub8["nb_mv"][0][2] = 1, 1, (-11, 26)
    assert sub8["has_uv"][0] == 1 and ipu.sub8x8(sub8[0], 4, 8)
    # the same kind of block lying the other way: 4 high, its upper neighbour inter on list 1 (the reference's chroma is defined here)
    sub8h = desc(8, 4, 32, 12, 0, (-9, 14), (0, 0), (1 << 16) | 2)
    sub8h["nb_is_inter"][0][1], sub8h["nb_list"][0][1], sub8h["nb_mv"][0][1] = 1, 1, (21, -6)
    assert sub8h["has_uv"][0] == 1 and ipu.sub8x8(sub8h[0], 8, 4)
    far = desc(8, 8, 64, 32, 0, (8 * (h + 90) + 5, 8 * (w + 70) + 3), (0, 0), (0 << 16) | 0)
    return [("uni_8x8", 8, 8, uni8), ("bi_16x16", 16, 16, bi16), ("uni_4x8_sub8x8_chroma", 4, 8, sub8), ("uni_8x4_sub8x8_chroma", 8, 4, sub8h),
            ("uni_8x8_into_border", 8, 8, far)]


def md_predict(refs8, bw, bh, desc):
    """The restatement of AV1InterPrediction10BitMD: the 8-bit prediction (tests/inter_pred_util.py) from the references' >> 2 planes, which
    is what Av1UnPackReferenceBlock hands the 8-bit convolution block by block.  refs8: two inter_pred_util.Picture.  Returns (y, cb, cr)"""
    import inter_pred_util as ipu
    w, h = MD_PIC
    pred = ipu.Picture(np.full((h, w), 0x55, np.uint8), np.full((h // 2, w // 2), 0x55, np.uint8), np.full((h // 2, w // 2), 0x55, np.uint8), 0)
    assert ipu.predict(refs8[0], refs8[1], pred, desc, bw, bh, 8) == 0
    return pred.y, pred.cb, pred.cr


def md_references8():
    """the 8-bit padded references the device chain has to arrive at: pad the 16-bit interiors, then >> 2"""
    import inter_pred_util as ipu
    return [ipu.Picture(*[unpack(pad_edges(p, MD_BORDER if k == 0 else MD_BORDER // 2))[0] for k, p in enumerate(planes)], MD_BORDER)
            for planes in md_reference_interiors()]


# ---------------------------------------------------------------------------------------------------------------------------------------
# plane sets with awkward geometry, and the device round trips (need torch and a GPU)

class PlaneSet:
    """n pictures' three planes in ONE flat array of `dtype`: every plane starts at an offset that is odd in samples (so never a multiple of
    16 bytes), its stride exceeds its width by an amount that is no multiple of 16 bytes, and everything outside the interiors is GUARD.
    `slack` = False packs the planes without any gap: strides equal the widths, offsets follow one another."""

    def __init__(self, planes_per_pic, dtype, slack=True, seed=0):
        self.dtype = np.dtype(dtype)
        self.guard = GUARD if self.dtype.itemsize == 1 else GUARD * 0x0101
        self.offsets, self.strides, self.shapes = [], [], []
        at = 0
        for j, planes in enumerate(planes_per_pic):
            offs, strs, shps = [], [], []
            for c, a in enumerate(planes):
                ph, pw = a.shape
                stride = pw + (5 + 2 * min(c, 1) + 4 * ((j + seed) % 3) if slack else 0)   # Cb and Cr share one, as svthip_inter_planes wants
                at += (7 + 2 * ((c + j + seed) % 4)) if slack else 0
                at |= 1 if slack else 0
                offs.append(at), strs.append(stride), shps.append((ph, pw))
                at += stride * ph
            self.offsets.append(offs), self.strides.append(strs), self.shapes.append(shps)
        self.size = at + (19 if slack else 0)
        self.host = np.full(self.size, self.guard, self.dtype)
        self.mask = np.zeros(self.size, bool)     # True inside the interiors
        for j, planes in enumerate(planes_per_pic):
            for c, a in enumerate(planes):
                self.view(self.host, j, c)[...] = a
                self.view(self.mask, j, c)[...] = True

    def view(self, flat, j, c):
        ph, pw = self.shapes[j][c]
        o, s = self.offsets[j][c], self.strides[j][c]
        return np.lib.stride_tricks.as_strided(flat[o:], (ph, pw), (s * flat.itemsize, flat.itemsize))

    def planes(self):
        """the svthip_planes array of the set"""
        import svtav1_hip
        return [svtav1_hip.make_planes(offs, strs) for offs, strs in zip(self.offsets, self.strides)]

    def upload(self):
        import torch
        self.dev = torch.from_numpy(self.host.view(np.uint8).copy()).to("cuda:0")
        return self.dev.data_ptr()

    def download(self):
        return self.dev.cpu().numpy().view(self.dtype)

    def check(self, want_per_pic, what):
        """after a call that wrote the set: the interiors are `want`, every other sample still GUARD"""
        got = self.download()
        assert (got[~self.mask] == self.guard).all(), f"{what}: wrote outside the interiors"
        for j, planes in enumerate(want_per_pic):
            for c, a in enumerate(planes):
                assert np.array_equal(self.view(got, j, c), a), f"{what}: picture {j} plane {PLANES[c]} differs"


class TiledSet:
    """n pictures' three compressed planes, one after the other behind an odd offset"""

    def __init__(self, tiled_per_pic):
        self.offsets, at = [], 3
        for planes in tiled_per_pic:
            offs = []
            for a in planes:
                offs.append(at)
                at += a.size + 1
            self.offsets.append(offs)
        self.host = np.full(at + 5, GUARD, np.uint8)
        for offs, planes in zip(self.offsets, tiled_per_pic):
            for o, a in zip(offs, planes):
                self.host[o:o + a.size] = a

    def planes(self):
        import svtav1_hip
        return [svtav1_hip.make_planes(offs, [0, 0, 0]) for offs in self.offsets]

    def upload(self):
        import torch
        self.dev = torch.from_numpy(self.host.copy()).to("cuda:0")
        return self.dev.data_ptr()


def blank_like(planes_per_pic, dtype):
    return [[np.zeros(a.shape, dtype) for a in planes] for planes in planes_per_pic]


def device_sse(ctx, recon_set, src_set, w, h, n, source_form=None, srcn_set=None):
    """[n][3] uint64 from svthip_picture_sse_dev (source_form None) or svthip_highbd_picture_sse_dev"""
    import torch
    d_sse = torch.full((n, 3), -1, dtype=torch.int64, device="cuda:0")
    d_recon, d_src = recon_set.upload(), src_set.upload()
    if source_form is None:
        ctx.picture_sse_dev(d_recon, recon_set.planes(), d_src, src_set.planes(), w, h, d_sse.data_ptr())
    else:
        d_srcn = srcn_set.upload() if srcn_set is not None else None
        ctx.highbd_picture_sse_dev(d_recon, recon_set.planes(), source_form, d_src, src_set.planes(), d_srcn,
                                   srcn_set.planes() if srcn_set is not None else None, w, h, d_sse.data_ptr())
    ctx.synchronize()
    return d_sse.cpu().numpy().view(np.uint64)
