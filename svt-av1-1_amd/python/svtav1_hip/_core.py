"""Loading libsvtav1_hip.so, its error type, and the context entries of include/svtav1_hip.h."""
from __future__ import annotations

import ctypes as C
import os

from . import _abi

_PKG_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
# SVTAV1_HIP_LIB: A/B tooling only (tools/kernel_times.py loads experimental builds of the library side by side)
LIB_PATH = os.environ.get("SVTAV1_HIP_LIB") or os.path.join(_PKG_ROOT, "libsvtav1_hip.so")

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)

_lib = None


def lib() -> C.CDLL:
    """Load libsvtav1_hip.so (built in-tree by `make -C svt-av1-1_amd` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built: run `make -C svt-av1-1_amd` (there is no CPU fallback)")
    # The PyTorch wheel bundles its own libamdhip64/libhsa-runtime64.  Two HIP runtimes in one process
    # cannot both own the GPU (measured: loading this library first makes torch report "No HIP GPUs"),
    # so when torch is installed it is imported first and this library binds to the runtime torch loaded.
    # A C host (the real integration) links the system ROCm runtime and never sees torch.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    _abi.bind(L)
    _lib = L
    return L


OPT_SADLOOP_GENERIC = _abi.define("SVTHIP_OPT_SADLOOP_GENERIC")
OPT_CONVOLVE_VALU = _abi.define("SVTHIP_OPT_CONVOLVE_VALU")
OPT_TQ_MAX_WORKGROUPS = _abi.define("SVTHIP_OPT_TQ_MAX_WORKGROUPS")


class SvtHipError(RuntimeError):
    pass


def _check(rc: int):
    if rc != 0:
        raise SvtHipError(f"svthip error 0x{rc & 0xFFFFFFFF:08x}: {lib().svthip_last_error().decode()}")


def _picture_ref(picture):
    return C.cast(C.byref(picture), C.c_void_p) if picture is not None else None


def _hbd(bit_depth, name):
    return (getattr(lib(), "svthip_av1_" + name), ()) if bit_depth == 8 else (getattr(lib(), "svthip_av1_highbd_" + name), (bit_depth,))


class ContextCore:
    """svthip_create / _destroy / _stream / _synchronize / _set_option / _reserve"""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().svthip_create(device, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().svthip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return lib().svthip_stream(self._h)

    def synchronize(self):
        _check(lib().svthip_synchronize(self._h))

    def set_option(self, option: int, value: int):
        """svthip_set_option: kernel-selection override of this context (OPT_SADLOOP_GENERIC / OPT_CONVOLVE_VALU / OPT_TQ_MAX_WORKGROUPS)."""
        _check(lib().svthip_set_option(self._h, option, value))

    def reserve(self, width: int, height: int, n_pu: int = 85, n_jobs: int = 1, host_forms: bool = False):
        _check(lib().svthip_reserve(self._h, width, height, n_pu, n_jobs, int(host_forms)))
