"""Host-pointer picture and TU forms (svthip_motion_estimate_picture / svthip_open_loop_intra_search_picture / svthip_encode_tu_batch)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._core import _check, lib
from ._tq import TU_DESC_DTYPE

# svthip_host_picture: a host luma plane (the caller keeps the buffer alive), the sample at (origin_x, origin_y) is picture (0, 0).
HostPicture = _abi.structure("svthip_host_picture")
# svthip_me_cu_result_ref: the reference's MeCuResults_t (40 bytes; `direction` words hold 0..2, padding is written as 0)
# hand-written: the recorded form leaves the trailing pad_[7] unnamed, the header names it
ME_CU_RESULT_REF_DTYPE = np.dtype({"names": ["xMvL0", "yMvL0", "xMvL1", "yMvL1", "distortionDirection", "totalMeCandidateIndex"],
                                   "formats": ["<i2", "<i2", "<i2", "<i2", (np.dtype([("distortion", "<u4"), ("direction", "<u4")]), (3,)), "u1"],
                                   "offsets": [0, 2, 4, 6, 8, 32], "itemsize": 40})


def _row_pointers(rows):
    return (C.c_void_p * rows.shape[0])(*[rows.ctypes.data + i * rows.strides[0] for i in range(rows.shape[0])])


class HostForms:
    """the host-pointer entries as Context methods"""

    def motion_estimate_picture(self, cur, ref0, ref1, params, use_subpel=True, cu8x8_mode=0, n_pu=85):
        """Whole-picture ME with host buffers (HostPicture cur / ref0 / ref1, ref1=None for P pictures; synchronous).  Returns the
        MeCuResults_t rows: ME_CU_RESULT_REF_DTYPE [n_sb][n_pu], SBs in raster order."""
        n_sb = ((cur.width + 63) // 64) * ((cur.height + 63) // 64)
        rows = np.zeros((n_sb, n_pu), ME_CU_RESULT_REF_DTYPE)
        _check(lib().svthip_motion_estimate_picture(self._h, C.byref(cur), C.byref(ref0), C.byref(ref1) if ref1 is not None else None, C.byref(params),
                                                    int(use_subpel), int(cu8x8_mode), n_pu, _row_pointers(rows)))
        return rows

    def open_loop_intra_search_picture(self, cur, params, me_rows=None, n_pu=85):
        """OpenLoopIntraSearchLcu over every SB of a HostPicture (synchronous).  me_rows: the [n_sb][n_pu] ME_CU_RESULT_REF_DTYPE rows of
        motion_estimate_picture, or None on the branches that do not read them.  Returns (cand [n_sb][85][18] u32, total [n_sb][85] u8)."""
        n_sb = ((cur.width + 63) // 64) * ((cur.height + 63) // 64)
        cand = np.zeros((n_sb, 85, 18), np.uint32)
        total = np.zeros((n_sb, 85), np.uint8)
        ptrs = None
        if me_rows is not None:
            assert me_rows.dtype == ME_CU_RESULT_REF_DTYPE and me_rows.shape == (n_sb, n_pu)
            ptrs = _row_pointers(me_rows)
        _check(lib().svthip_open_loop_intra_search_picture(self._h, C.byref(cur), C.byref(params), ptrs, n_pu, cand.ctypes.data, total.ctypes.data))
        return cand, total

    def encode_tu_batch(self, src, pred, recon, desc, tx_width, tx_height, qparams, iscan, coeff_samples):
        """The fused T/Q chain with host buffers (synchronous).  src / pred / recon: contiguous planes of one dtype, uint8 or uint16 (16-bit
        planes); recon may be pred itself (in-place reconstruction) and is written in place.  Returns dict coeff / qcoeff / dqcoeff (int32
        [coeff_samples]), eob (uint16 [n]), energy (uint64 [n]), dist (uint64 [n][2])."""
        assert src.dtype in (np.uint8, np.uint16) and pred.dtype == recon.dtype == src.dtype and pred.size == recon.size == src.size
        assert all(a.flags.c_contiguous for a in (src, pred, recon))
        desc = np.ascontiguousarray(desc, TU_DESC_DTYPE)
        qparams = np.ascontiguousarray(qparams, np.int16).reshape(-1, 10)
        iscan = np.ascontiguousarray(iscan, np.int16)
        n = len(desc)
        out = {"coeff": np.zeros(coeff_samples, np.int32), "qcoeff": np.zeros(coeff_samples, np.int32), "dqcoeff": np.zeros(coeff_samples, np.int32),
               "eob": np.zeros(n, np.uint16), "energy": np.zeros(n, np.uint64), "dist": np.zeros((n, 2), np.uint64)}
        _check(lib().svthip_encode_tu_batch(self._h, src.ctypes.data, pred.ctypes.data, recon.ctypes.data, src.size, int(src.dtype == np.uint16),
                                            desc.ctypes.data, n, tx_width, tx_height, qparams.ctypes.data, qparams.shape[0], iscan.ctypes.data, iscan.size,
                                            coeff_samples, out["coeff"].ctypes.data, out["qcoeff"].ctypes.data, out["dqcoeff"].ctypes.data,
                                            out["eob"].ctypes.data, out["energy"].ctypes.data, out["dist"].ctypes.data))
        return out
