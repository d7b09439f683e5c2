"""Writes tests/golden/bitdepth.npz from the reference's own UnPack2D, extract_8bit_data, Pack2D_SRC, CompressedPackLcu, PsnrCalculations and
AV1InterPrediction10BitMD (tests/golden/ref_bitdepth_driver.c, linked by the recipe of oracle/ref_driver.py against the reference objects of
the oracle build, oracle/_ref/obj_all).  Run in the build container only, where the reference exists: the fixture is data.

    python tests/golden/make_golden_bitdepth.py

Cases (tests/bitdepth_util.py CASES): 72x40 (a full SB column and one 8 wide, SB height 40, chroma SB widths 32 and 4) and 136x72 (compressed
rows of 34 and 17 bytes, a second SB row 8 high), three constructed pictures each (bitdepth_util.make_pictures: clean 10-bit, bits above bit
9 set, random words) and one picture of maximal differences.  Contents, planes pl = y, cb, cr:
  case [2][2]                                     width, height
  c{c}_p{i}_{in16,inn,tiled,recon8,recon16}_{pl}  the inputs: 16-bit input, dirty unpacked 2-bit plane, compressed plane, reconstructions
  c{c}_p{i}_{out8,outn}_{pl}                      UnPack2D of in16 (extract_8bit_data is asserted to give out8 and is not stored)
  c{c}_p{i}_pack16_{pl}                           Pack2D_SRC of (out8, inn), SB by SB
  c{c}_p{i}_packc16_{pl}                          CompressedPackLcu of (out8, tiled), SB by SB
  c{c}_p{i}_{sse8,sse16_unpacked,sse16_compressed}  [3] u32: luma_sse, cb_sse, cr_sse as PsnrCalculations leaves them (truncated, Cb / Cr
                                                  swapped) for recon8 against out8, recon16 against (out8, inn) and against (out8, tiled)
  c{c}_max_*                                      the same inputs and three SSE results of the maximal-difference picture
  md_{name}_{desc,ref_frame_type,nb_frame}        one PU of bitdepth_util.md_cases() and the frame types given to the reference
  md_{name}_pred_{pl}                             AV1InterPrediction10BitMD's 8-bit prediction from the edge-padded 10-bit references of
                                                  bitdepth_util.md_reference_interiors() (computed, not stored), planes pre-filled with 0x55
The restatement (tests/bitdepth_util.py) is asserted equal to everything stored."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "svt-av1-1_amd", "python"), ROOT]

import bitdepth_util as bu  # noqa: E402
import inter_pred_util as ipu  # noqa: E402
from make_golden_cdef import save  # noqa: E402
from oracle import ref_driver  # noqa: E402
from oracle.ref_driver import reference_available  # noqa: E402

INTRA, LAST, BWDREF = 0, 1, 5
V = C.c_void_p


def build_driver(out_dir):
    """ref_bitdepth_driver.c by the recipe of oracle/ref_driver.py, with its signatures"""
    L = ref_driver.build_driver(os.path.join(HERE, "ref_bitdepth_driver.c"), out_dir)
    L.drv_unpack.argtypes = [C.c_int, C.c_int, V, V, V]
    L.drv_extract8.argtypes = [C.c_int, C.c_int, V, V]
    L.drv_pack.argtypes = [C.c_int, C.c_int, C.c_int, V, V, V]
    L.drv_psnr.argtypes = [C.c_int, C.c_int, C.c_int, V, V, V, V]
    L.drv_md_predict.argtypes = [V, V, C.c_int, C.c_int, V, V, C.c_int, C.c_int, C.c_int]
    for f in (L.drv_unpack, L.drv_extract8, L.drv_pack, L.drv_psnr):
        f.restype = None
    L.drv_init()
    return L


def _ptrs(planes):
    for a in planes:
        assert a.flags.c_contiguous
    return (V * len(planes))(*[a.ctypes.data for a in planes])


def _like(planes, dtype, fill=0):
    return [np.full(a.shape, fill, dtype) for a in planes]


def reference_forms(L, w, h, in16, inn, tiled):
    """out8, outn, pack16, packc16 of one picture from the driver"""
    in16 = [np.ascontiguousarray(a) for a in in16]
    out8, outn, alone = _like(in16, np.uint8), _like(in16, np.uint8), _like(in16, np.uint8)
    L.drv_unpack(w, h, _ptrs(in16), _ptrs(out8), _ptrs(outn))
    L.drv_extract8(w, h, _ptrs(in16), _ptrs(alone))
    assert all(np.array_equal(a, b) for a, b in zip(alone, out8)), "extract_8bit_data and UnPack2D disagree on the 8-bit plane"
    pack16, packc16 = _like(in16, np.uint16, 0xdead), _like(in16, np.uint16, 0xdead)
    L.drv_pack(0, w, h, _ptrs(out8), _ptrs([np.ascontiguousarray(a) for a in inn]), _ptrs(pack16))
    L.drv_pack(1, w, h, _ptrs(out8), _ptrs([np.ascontiguousarray(a) for a in tiled]), _ptrs(packc16))
    return {"out8": out8, "outn": outn, "pack16": pack16, "packc16": packc16}


def reference_sse(L, w, h, in8, inn, tiled, recon8, recon16):
    """the three fields PsnrCalculations leaves, per arm"""
    out = {}
    for k, mode, recon, srcn in (("sse8", 0, recon8, None), ("sse16_unpacked", 1, recon16, inn), ("sse16_compressed", 2, recon16, tiled)):
        o = np.zeros(3, np.uint32)
        L.drv_psnr(mode, w, h, _ptrs([np.ascontiguousarray(a) for a in recon]), _ptrs([np.ascontiguousarray(a) for a in in8]),
                   _ptrs([np.ascontiguousarray(a) for a in srcn]) if srcn is not None else None, o.ctypes.data)
        out[k] = o
    return out


def md_references16():
    return [ipu.Picture(*[np.ascontiguousarray(bu.pad_edges(p, bu.MD_BORDER if k == 0 else bu.MD_BORDER // 2)) for k, p in enumerate(planes)],
                        bu.MD_BORDER) for planes in bu.md_reference_interiors()]


def reference_md_predict(L, refs16, bw, bh, desc, local_fill=0):
    """AV1InterPrediction10BitMD of the one PU of `desc`: (y, cb, cr), the ref_frame_type and the neighbours' frames handed over.
    local_fill: what the function's two local 8-bit block buffers hold before the call"""
    w, h = bu.MD_PIC
    d = desc[0]
    pred = [np.full((h, w), 0x55, np.uint8), np.full((h // 2, w // 2), 0x55, np.uint8), np.full((h // 2, w // 2), 0x55, np.uint8)]
    arrs = [refs16[0].y, refs16[0].cb, refs16[0].cr, refs16[1].y, refs16[1].cb, refs16[1].cr, *pred]
    strides = np.array([refs16[0].y.shape[1], refs16[0].cb.shape[1], refs16[1].y.shape[1], refs16[1].cb.shape[1], w, w // 2], np.int32)
    rft = {0: LAST, 1: BWDREF, 2: 8}[int(d["pred_direction"])]
    pu = np.array([d["pu_origin_x"], d["pu_origin_y"], d["dst_origin_x"], d["dst_origin_y"], bw, bh, ipu.SIZES.index((bw, bh)), d["interp_filters"], rft,
                   d["pred_direction"], d["mv"][0][0], d["mv"][0][1], d["mv"][1][0], d["mv"][1][1], d["mb_to_left_edge"], d["mb_to_right_edge"],
                   d["mb_to_top_edge"], d["mb_to_bottom_edge"], d["has_uv"]], np.int64).astype(np.int32)
    nb = np.zeros(9, np.int32)
    for k in range(3):
        nb[3 * k] = INTRA if not d["nb_is_inter"][k] else (LAST if d["nb_list"][k] == 0 else BWDREF)
        nb[3 * k + 1], nb[3 * k + 2] = d["nb_mv"][k]
    assert L.drv_md_predict(pu.ctypes.data, nb.ctypes.data, w, h, _ptrs(arrs), strides.ctypes.data, refs16[0].border, 0, local_fill) == 0
    return pred, rft, nb[0::3].copy()


def reference_md_case(L, refs16, bw, bh, desc):
    """(prediction, ref_frame_type, neighbour frames, chroma_defined).  The call is made twice, its local block buffers holding 0x00 and then
    0xFF beforehand: a plane on which the two runs differ is a plane the reference computes from bytes it never wrote (see
    bitdepth_util.MD_UNDEFINED_NOTE) -- the luma never is; chroma_defined says whether Cb and Cr are the same in both runs"""
    a, rft, nb_frame = reference_md_predict(L, refs16, bw, bh, desc, 0x00)
    b, _, _ = reference_md_predict(L, refs16, bw, bh, desc, 0xFF)
    assert np.array_equal(a[0], b[0]), "the luma prediction depends on the local buffer's earlier contents"
    return a, rft, nb_frame, bool(np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]))


def main():
    assert reference_available(), "needs the reference sources and oracle/_ref/obj_all (python -c 'import __graft_entry__ as g; g.build()')"
    rng = np.random.default_rng(20261020)
    out = {"case": np.array(bu.CASES, np.int32)}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for c, (w, h) in enumerate(bu.CASES):
            for i, p in enumerate(bu.make_pictures(rng, w, h)):
                ref = reference_forms(L, w, h, p["in16"], p["inn"], p["tiled"])
                ref.update(reference_sse(L, w, h, ref["out8"], p["inn"], p["tiled"], p["recon8"], p["recon16"]))
                mine = bu.expected(p)
                for k in ("out8", "outn", "pack16", "packc16"):
                    for pl in range(3):
                        assert np.array_equal(mine[k][pl], ref[k][pl]), ("the restatement differs from the reference", (w, h), i, k, pl)
                        out[f"c{c}_p{i}_{k}_{bu.PLANES[pl]}"] = ref[k][pl]
                for k in ("sse8", "sse16_unpacked", "sse16_compressed"):
                    assert np.array_equal(bu.reference_fields(mine[k]), ref[k]), ("the restatement differs from the reference", (w, h), i, k, mine[k], ref[k])
                    out[f"c{c}_p{i}_{k}"] = ref[k]
                for k in ("in16", "inn", "tiled", "recon8", "recon16"):
                    for pl in range(3):
                        out[f"c{c}_p{i}_{k}_{bu.PLANES[pl]}"] = p[k][pl]
                print("case", c, (w, h), "picture", i, {k: [int(v) for v in mine[k]] for k in ("sse8", "sse16_unpacked", "sse16_compressed")})
            p = bu.max_difference_picture(w, h, rng)
            ref = reference_sse(L, w, h, p["in8"], p["inn"], p["tiled"], p["recon8"], p["recon16"])
            want = bu.expected_max_difference(p)
            for k in want:
                assert np.array_equal(bu.reference_fields(want[k]), ref[k]), ("maximal differences", (w, h), k, want[k], ref[k])
                out[f"c{c}_max_{k}"] = ref[k]
            for k in ("in8", "inn", "tiled", "recon8", "recon16"):
                for pl in range(3):
                    out[f"c{c}_max_{k}_{bu.PLANES[pl]}"] = p[k][pl]
            print("case", c, (w, h), "maximal differences", {k: [int(v) for v in want[k]] for k in want}, "fields", ref)
        refs16, refs8 = md_references16(), bu.md_references8()
        for name, bw, bh, desc in bu.md_cases():
            pred, rft, nb_frame, chroma_defined = reference_md_case(L, refs16, bw, bh, desc)
            assert chroma_defined == (name not in bu.MD_CHROMA_UNDEFINED), (name, chroma_defined)
            mine = bu.md_predict(refs8, bw, bh, desc)
            for pl in range(3):
                if pl == 0 or chroma_defined:
                    assert np.array_equal(mine[pl], pred[pl]), ("the 8-bit prediction from >> 2 references differs from AV1InterPrediction10BitMD", name, pl)
                    out[f"md_{name}_pred_{bu.PLANES[pl]}"] = pred[pl]
            out[f"md_{name}_desc"], out[f"md_{name}_ref_frame_type"], out[f"md_{name}_nb_frame"] = desc, np.int32(rft), nb_frame
            print("md", name, "samples written", [int((a != 0x55).sum()) for a in pred], "chroma defined" if chroma_defined else "chroma UNDEFINED")
    save(bu.FIXTURE, out)
    print(f"wrote {bu.FIXTURE}: {os.path.getsize(bu.FIXTURE) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
