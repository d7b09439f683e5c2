"""The five film-grain estimation entries are declared in include/svtav1_hip.h, exported by the library and bound by the package from the
header; the header compiles as C99 and its state and feature structs have the sizes the binding derives (no GPU needed).  The refusals need
a context and are marked gpu: nothing is launched and the outputs keep what they held."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import abi_util  # noqa: E402

ENTRIES = {"svthip_film_grain_noise_model_dev": 12, "svthip_highbd_film_grain_noise_model_dev": 13, "svthip_film_grain_flat_block_tables_dev": 3,
           "svthip_film_grain_flat_block_features_dev": 10, "svthip_highbd_film_grain_flat_block_features_dev": 11}
METHODS = ("film_grain_noise_model_dev", "highbd_film_grain_noise_model_dev", "film_grain_flat_block_tables_dev", "film_grain_flat_block_features_dev",
           "highbd_film_grain_flat_block_features_dev")
BAD = "80001005"
CHANNEL_BYTES = 8 * (625 + 25 + 25 + 1 + 400 + 20 + 20 + 1) + 8


def test_header_declares_library_exports_and_package_binds_every_entry():
    import svtav1_hip
    full = open(os.path.join(ROOT, "include", "svtav1_hip.h")).read()
    declared = set(re.findall(r"\b(svthip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", full, flags=re.S)))
    lib = ctypes.CDLL(svtav1_hip.LIB_PATH)
    for n, n_args in ENTRIES.items():
        assert n in declared, f"{n} is not declared in include/svtav1_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        fn = getattr(svtav1_hip.lib(), n)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args and fn.restype is ctypes.c_int32, n
    for m in METHODS:
        assert callable(getattr(svtav1_hip.Context, m, None)), m
    # the section cites the reference lines the entries replace and says what stays on the host
    section = full[full.index("Film-grain ESTIMATION"):full.index("svthip_highbd_film_grain_flat_block_features_dev(")]
    for cite in ("noise_model.c:1744-1822", ":1030-1147", ":580-686", "aom_wiener_denoise_2d", "aom_noise_model_save_latest", "aom_noise_model_get_grain_parameters",
                 "NOT device-resident", ":843-853", ":914", "mathutils.h:26-60", ":238-247", ":314-350", "mean / 8192", ":483-510", "DENOISING_BlockSize"):
        assert cite in section, cite


def test_header_compiles_as_c99_and_the_struct_sizes_match_the_binding(tmp_path):
    import svtav1_hip
    src = tmp_path / "decl.c"
    src.write_text('#include "svtav1_hip.h"\ntypedef void (*fp)(void);\nfp entries[5] = {' + ", ".join(f"(fp){n}" for n in ENTRIES) + "};\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "decl.o"), str(src)])
    lay = tmp_path / "size.c"
    lay.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svtav1_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(svthip_film_grain_noise_channel), sizeof(svthip_film_grain_noise_state),\n'
                   "         offsetof(svthip_film_grain_noise_state, combined), offsetof(svthip_film_grain_noise_state, status),\n"
                   "         offsetof(svthip_film_grain_noise_channel, strength_A), sizeof(svthip_film_grain_flat_block_features));\n  return 0;\n}\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(lay)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [CHANNEL_BYTES, 6 * CHANNEL_BYTES + 8, 3 * CHANNEL_BYTES, 6 * CHANNEL_BYTES, 8 * 676, 32]
    state, feat = svtav1_hip.film_grain_noise_state_dtype(), svtav1_hip.film_grain_flat_block_features_dtype()
    abi_util.assert_sizes((state, 6 * CHANNEL_BYTES + 8), (feat, 32))
    assert state.fields["combined"][1] == 3 * CHANNEL_BYTES and state.fields["status"][1] == 6 * CHANNEL_BYTES and feat.names == ("trace", "ratio", "norm", "var")
    assert state["latest"].base.fields["strength_A"][1] == 8 * 676 and state["latest"].shape == (3,)
    assert (svtav1_hip.FILM_GRAIN_NOISE_BLOCK_SIZE, svtav1_hip.FILM_GRAIN_NOISE_LAG, svtav1_hip.FILM_GRAIN_NOISE_SHAPE_SQUARE) == (32, 3, 1)
    assert (svtav1_hip.FILM_GRAIN_NOISE_OK, svtav1_hip.FILM_GRAIN_NOISE_INSUFFICIENT_FLAT_BLOCKS, svtav1_hip.FILM_GRAIN_NOISE_INTERNAL_ERROR) == (0, 2, 4)
    assert svtav1_hip.FILM_GRAIN_FLAT_TABLES_DOUBLES == 1024 * 3 + 9


def test_the_glue_includes_its_two_headers_alone():
    text = open(os.path.join(ROOT, "svt-av1-1_amd", "csrc", "fg_abi.hip")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["svthip_glue.h", "fg_launch.h"]


def test_a_null_context_is_refused():
    import svtav1_hip
    lib = svtav1_hip.lib()
    bad = int(BAD, 16)
    three = (ctypes.c_void_p * 3)(8, 8, 8)
    stride = (ctypes.c_uint32 * 3)(64, 32, 32)
    assert lib.svthip_film_grain_noise_model_dev(None, three, three, stride, 64, 64, 32, 3, 1, 8, 8, None) & 0xFFFFFFFF == bad
    assert lib.svthip_highbd_film_grain_noise_model_dev(None, three, three, stride, 64, 64, 10, 32, 3, 1, 8, 8, None) & 0xFFFFFFFF == bad
    assert lib.svthip_film_grain_flat_block_tables_dev(None, 8, None) & 0xFFFFFFFF == bad
    assert lib.svthip_film_grain_flat_block_features_dev(None, 8, 64, 64, 64, 32, None, 8, 8, None) & 0xFFFFFFFF == bad
    assert lib.svthip_highbd_film_grain_flat_block_features_dev(None, 8, 64, 64, 64, 10, 32, None, 8, 8, None) & 0xFFFFFFFF == bad


@pytest.mark.gpu
def test_refused_arguments(hip_ctx):
    """the library's error, and nothing launched: state, features, bytes and tables keep what they held"""
    torch = pytest.importorskip("torch")
    import svtav1_hip
    import fg_model_util as mu
    ctx = hip_ctx
    w, h = 64, 64
    runs = {}
    for p, bd in ((0, 8), (2, 10)):
        data, den = mu.planes_of(p)
        hh, ww = data[0].shape
        dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in (*data, *den)]
        runs[bd] = (ww, hh, dev, [t.data_ptr() for t in dev[:3]], [t.data_ptr() for t in dev[3:]], [ww, ww // 2, ww // 2])
    d_flat = torch.full((16,), 255, dtype=torch.uint8, device="cuda:0")
    d_state = torch.full((mu.STATE.itemsize,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_feat = torch.full((16 * 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_is = torch.full((16,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_tab = torch.full((mu.TABLES_DOUBLES * 8,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def model(bd, **kw):
        ww, hh, _, data, den, stride = runs[bd]
        a = dict(d_data=data, d_denoised=den, stride=stride, width=ww, height=hh, d_flat_blocks=d_flat.data_ptr(), d_state=d_state.data_ptr())
        a.update(kw)
        if bd == 8:
            ctx.film_grain_noise_model_dev(**a)
        else:
            ctx.highbd_film_grain_noise_model_dev(bit_depth=a.pop("bit_depth", 10), **a)

    def feats(bd, **kw):
        ww, hh, _, data, _, _ = runs[bd]
        a = dict(d_luma=data[0], stride=ww, width=ww, height=hh, d_features=d_feat.data_ptr(), d_is_flat=d_is.data_ptr())
        a.update(kw)
        if bd == 8:
            ctx.film_grain_flat_block_features_dev(**a)
        else:
            ctx.highbd_film_grain_flat_block_features_dev(bit_depth=a.pop("bit_depth", 10), **a)

    refused = []
    for bd in (8, 10):
        ww, hh, _, data, den, stride = runs[bd]
        refused += [lambda bd=bd: model(bd, block_size=16), lambda bd=bd: model(bd, block_size=64), lambda bd=bd: model(bd, lag=2), lambda bd=bd: model(bd, lag=4),
                    lambda bd=bd: model(bd, shape=0), lambda bd=bd, s=stride, ww=ww: model(bd, stride=[ww - 1, s[1], s[2]]),
                    lambda bd=bd, s=stride, ww=ww: model(bd, stride=[s[0], s[1], ww // 2 - 1]), lambda bd=bd, d=data: model(bd, d_data=[d[0], None, d[2]]),
                    lambda bd=bd, d=den: model(bd, d_denoised=[None, d[1], d[2]]), lambda bd=bd: model(bd, d_data=None), lambda bd=bd: model(bd, stride=None),
                    lambda bd=bd: model(bd, d_flat_blocks=None), lambda bd=bd: model(bd, d_state=None), lambda bd=bd: model(bd, d_state=d_state.data_ptr() + 4),
                    lambda bd=bd, ww=ww: model(bd, width=ww + 1), lambda bd=bd: model(bd, height=0),
                    lambda bd=bd: feats(bd, block_size=16), lambda bd=bd, ww=ww: feats(bd, stride=ww - 2), lambda bd=bd: feats(bd, d_luma=None),
                    lambda bd=bd: feats(bd, d_features=None), lambda bd=bd: feats(bd, d_is_flat=None), lambda bd=bd: feats(bd, width=0),
                    lambda bd=bd, hh=hh: feats(bd, height=hh + 1), lambda bd=bd: feats(bd, d_tables=d_tab.data_ptr() + 4)]
    refused += [lambda: model(10, bit_depth=12), lambda: model(10, bit_depth=8), lambda: feats(10, bit_depth=12), lambda: feats(10, bit_depth=8),
                lambda: model(10, d_data=[runs[10][3][0] + 1, runs[10][3][1], runs[10][3][2]]), lambda: feats(10, d_luma=runs[10][3][0] + 1),
                lambda: ctx.film_grain_flat_block_tables_dev(None), lambda: ctx.film_grain_flat_block_tables_dev(d_tab.data_ptr() + 4)]
    for i, call in enumerate(refused):
        with pytest.raises(svtav1_hip.SvtHipError, match=BAD):
            call()
            pytest.fail(f"refusal {i} was accepted")
    ctx.synchronize()
    for t in (d_state, d_feat, d_is, d_tab):
        assert (t.cpu().numpy() == 0x5A).all()
    assert w == runs[8][0] and h == runs[8][1]
