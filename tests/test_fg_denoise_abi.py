"""The film-grain Wiener denoising entries are declared in include/svtav1_hip.h, exported by the library and bound by the package from the
header, which compiles as C99; their signatures carry no struct; the two host functions answer without a context (no GPU needed; the
default psd crosses as pointers to float, the scalar forms the binding reads from the header being integers).  The
refusals need a context and are marked gpu: nothing is launched and the outputs keep what they held."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ENTRIES = {"svthip_film_grain_wiener_filter_dev": 9, "svthip_highbd_film_grain_wiener_filter_dev": 10, "svthip_film_grain_dither_dev": 8,
           "svthip_highbd_film_grain_dither_dev": 9, "svthip_film_grain_wiener_denoise_dev": 10, "svthip_highbd_film_grain_wiener_denoise_dev": 11}
HOST = {"svthip_film_grain_wiener_workspace_bytes": (2, ctypes.c_size_t), "svthip_film_grain_noise_psd_default": (3, ctypes.c_int32)}
METHODS = ("film_grain_wiener_filter_dev", "highbd_film_grain_wiener_filter_dev", "film_grain_dither_dev", "highbd_film_grain_dither_dev",
           "film_grain_wiener_denoise_dev", "highbd_film_grain_wiener_denoise_dev")
BAD = "80001005"


def test_header_declares_library_exports_and_package_binds_every_entry():
    import svtav1_hip
    full = open(os.path.join(ROOT, "include", "svtav1_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    declared = set(re.findall(r"\b(svthip_[a-z0-9_]+)\s*\(", code))
    lib = ctypes.CDLL(svtav1_hip.LIB_PATH)
    for n, n_args in ENTRIES.items():
        assert n in declared and hasattr(lib, n), n
        fn = getattr(svtav1_hip.lib(), n)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args and fn.restype is ctypes.c_int32, n
        proto = re.search(r"\b" + n + r"\s*\(([^)]*)\)", code).group(1)
        assert "struct" not in proto and not re.search(r"\bsvthip_(?!ctx\b)\w+", proto), f"{n} takes a struct"
    for n, (n_args, ret) in HOST.items():
        assert n in declared and hasattr(lib, n), n
        fn = getattr(svtav1_hip.lib(), n)
        assert len(fn.argtypes) == n_args and fn.restype is ret, n
    for m in METHODS:
        assert callable(getattr(svtav1_hip.Context, m, None)), m
    # the section cites the reference lines the entries replace; the estimation section no longer sends the filter to the host
    section = full[full.index("Film-grain Wiener DENOISING"):full.index("svthip_highbd_film_grain_wiener_denoise_dev(")]
    for cite in ("noise_model.c:1363-1500", ":522-563", ":1314-1326", "fft.c:58-72", ":114-184", "vec_size 8", "noise_util.c:93-112", ":1455-1466", ":1328-1361",
                 "fg_cos_window.inc", "denormals are kept", "no float atomics", "no workgroup waits on another"):
        assert cite in section, cite
    estimation = full[full.index("Film-grain ESTIMATION"):full.index("Film-grain Wiener DENOISING")]
    assert "is on the device too" in estimation and "exp(" in estimation and "aom_noise_model_save_latest" in estimation and "aom_noise_model_get_grain_parameters" in estimation


def test_header_compiles_as_c99_with_the_entries(tmp_path):
    src = tmp_path / "decl.c"
    names = list(ENTRIES) + list(HOST)
    src.write_text('#include "svtav1_hip.h"\ntypedef void (*fp)(void);\nfp entries[%d] = {' % len(names) + ", ".join(f"(fp){n}" for n in names) + "};\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "decl.o"), str(src)])


def test_host_functions():
    """the workspace is three planes of the reference's `result`; the default psd is the reference's formula in float"""
    import svtav1_hip
    import fg_denoise_util as du
    for w, h in ((64, 64), (100, 72), (36, 66), (1920, 1080), (3840, 2160)):
        pitch, rows = du.result_geometry(w, h)
        assert svtav1_hip.film_grain_wiener_workspace_bytes(w, h) == 3 * 4 * pitch * rows
    for n in (16, 32):
        for f in (5.0, 0.5, 1.3, 7.25, 50.0):
            assert np.float32(svtav1_hip.film_grain_noise_psd_default(n, f)).view(np.uint32) == du.psd_default(n, f).view(np.uint32), (n, f)


def test_the_kernels_generated_table_is_what_the_tool_renders():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_fg_cos_window as g
    table = g.read_table()
    assert len(table) == 48 and open(g.path()).read() == g.render(table)
    # a half-cosine: symmetric, rising to the middle, within (0, 1)
    for t in (table[:32], table[32:]):
        assert all(0 < v < 1 for v in t) and all(a < b for a, b in zip(t[:len(t) // 2 - 1], t[1:len(t) // 2])) and np.allclose(t, t[::-1], rtol=0, atol=1e-15)


def test_a_null_context_is_refused():
    import svtav1_hip
    lib = svtav1_hip.lib()
    bad = int(BAD, 16)
    three = (ctypes.c_void_p * 3)(8, 8, 8)
    stride = (ctypes.c_uint32 * 3)(64, 32, 32)
    assert lib.svthip_film_grain_wiener_filter_dev(None, three, stride, 64, 64, 32, three, 8, None) & 0xFFFFFFFF == bad
    assert lib.svthip_highbd_film_grain_wiener_filter_dev(None, three, stride, 64, 64, 10, 32, three, 8, None) & 0xFFFFFFFF == bad
    assert lib.svthip_film_grain_dither_dev(None, 8, three, stride, 64, 64, 32, None) & 0xFFFFFFFF == bad
    assert lib.svthip_highbd_film_grain_dither_dev(None, 8, three, stride, 64, 64, 10, 32, None) & 0xFFFFFFFF == bad
    assert lib.svthip_film_grain_wiener_denoise_dev(None, three, stride, three, stride, 64, 64, 32, three, None) & 0xFFFFFFFF == bad
    assert lib.svthip_highbd_film_grain_wiener_denoise_dev(None, three, stride, three, stride, 64, 64, 10, 32, three, None) & 0xFFFFFFFF == bad


@pytest.mark.gpu
def test_refused_arguments(hip_ctx):
    """the library's error, and nothing launched: float planes and samples keep what they held"""
    torch = pytest.importorskip("torch")
    import svtav1_hip
    import fg_denoise_util as du
    ctx = hip_ctx
    runs = {}
    for p, bd in ((0, 8), (2, 10)):
        data = du.planes_of(p)
        hh, ww = data[0].shape
        src = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in data]
        dst = [torch.full((t.numel(),), 0x5A, dtype=torch.uint8, device="cuda:0") for t in src]
        runs[bd] = (ww, hh, src, dst, [t.data_ptr() for t in src], [t.data_ptr() for t in dst], [ww, ww // 2, ww // 2])
    psd_t = [torch.zeros(1024, dtype=torch.float32, device="cuda:0") for _ in range(3)]
    psd = [t.data_ptr() for t in psd_t]
    planes = torch.full((svtav1_hip.film_grain_wiener_workspace_bytes(96, 64),), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def filt(bd, **kw):
        ww, hh, _, _, s, _, stride = runs[bd]
        a = dict(d_data=s, stride=stride, width=ww, height=hh, d_noise_psd=psd, d_planes=planes.data_ptr())
        a.update(kw)
        if bd == 8:
            ctx.film_grain_wiener_filter_dev(**a)
        else:
            ctx.highbd_film_grain_wiener_filter_dev(bit_depth=a.pop("bit_depth", 10), **a)

    def dith(bd, **kw):
        ww, hh, _, _, _, d, stride = runs[bd]
        a = dict(d_planes=planes.data_ptr(), d_denoised=d, stride=stride, width=ww, height=hh)
        a.update(kw)
        if bd == 8:
            ctx.film_grain_dither_dev(**a)
        else:
            ctx.highbd_film_grain_dither_dev(bit_depth=a.pop("bit_depth", 10), **a)

    def both(bd, **kw):
        ww, hh, _, _, s, d, stride = runs[bd]
        a = dict(d_data=s, data_stride=stride, d_denoised=d, denoised_stride=stride, width=ww, height=hh, d_noise_psd=psd)
        a.update(kw)
        if bd == 8:
            ctx.film_grain_wiener_denoise_dev(**a)
        else:
            ctx.highbd_film_grain_wiener_denoise_dev(bit_depth=a.pop("bit_depth", 10), **a)

    refused = []
    for bd in (8, 10):
        ww, hh, _, _, s, d, stride = runs[bd]
        for call, planes_key, stride_key in ((filt, "d_data", "stride"), (dith, "d_denoised", "stride"), (both, "d_data", "data_stride"), (both, "d_denoised", "denoised_stride")):
            ptrs = d if planes_key == "d_denoised" else s
            refused += [lambda c=call, bd=bd: c(bd, block_size=16), lambda c=call, bd=bd: c(bd, block_size=64), lambda c=call, bd=bd: c(bd, width=0),
                        lambda c=call, bd=bd, ww=ww: c(bd, width=ww + 1), lambda c=call, bd=bd, hh=hh: c(bd, height=hh + 1), lambda c=call, bd=bd: c(bd, height=0),
                        lambda c=call, bd=bd: c(bd, width=65538), lambda c=call, bd=bd: c(bd, height=65538),
                        lambda c=call, bd=bd, k=stride_key, st=stride, ww=ww: c(bd, **{k: [ww - 1, st[1], st[2]]}),
                        lambda c=call, bd=bd, k=stride_key, st=stride, ww=ww: c(bd, **{k: [st[0], st[1], ww // 2 - 1]}),
                        lambda c=call, bd=bd, k=stride_key: c(bd, **{k: None}), lambda c=call, bd=bd, k=planes_key: c(bd, **{k: None}),
                        lambda c=call, bd=bd, k=planes_key, q=ptrs: c(bd, **{k: [q[0], None, q[2]]})]
        for call in (filt, both):
            refused += [lambda c=call, bd=bd: c(bd, d_noise_psd=None), lambda c=call, bd=bd: c(bd, d_noise_psd=[psd[0], psd[1], None]),
                        lambda c=call, bd=bd: c(bd, d_noise_psd=[psd[0] + 2, psd[1], psd[2]])]
        for call in (filt, dith):
            refused += [lambda c=call, bd=bd: c(bd, d_planes=None), lambda c=call, bd=bd: c(bd, d_planes=planes.data_ptr() + 2)]
    for call, key, which in ((filt, "d_data", 4), (dith, "d_denoised", 5), (both, "d_data", 4), (both, "d_denoised", 5)):
        q = runs[10][which]
        refused += [lambda c=call: c(10, bit_depth=12), lambda c=call: c(10, bit_depth=8), lambda c=call, k=key, q=q: c(10, **{k: [q[0] + 1, q[1], q[2]]})]
    for i, call in enumerate(refused):
        with pytest.raises(svtav1_hip.SvtHipError, match=BAD):
            call()
            pytest.fail(f"refusal {i} was accepted")
    ctx.synchronize()
    assert (planes.cpu().numpy() == 0x5A).all()
    for bd in (8, 10):
        for t in runs[bd][3]:
            assert (t.cpu().numpy() == 0x5A).all()
