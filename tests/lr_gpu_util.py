"""GPU test helpers of the loop-restoration tests (tests/test_lr_gpu.py, tests/test_lr_sgr_gpu.py): planes inside guarded allocations, a
fixture case on the device with its workspace.
The context's stream does not wait for torch's: a tensor that torch fills on its own stream (torch.full, fill_, zeros) is only safe to hand
to an entry after _ready(), or the tail of the fill can land on what the kernel has already written.  (_dev copies from pageable host
memory and has landed when it returns.)"""
import numpy as np

import svtav1_hip

GUARD = 9   # samples of guard around every plane, odd so that the planes start unaligned to a dword row
FILL = {8: 0xA5, 10: 0x2A5}


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _ready(torch):
    """torch's fills have landed: the library's stream does not order itself behind them"""
    torch.cuda.synchronize()


class Guarded:
    """three planes embedded in larger allocations filled with a guard pattern; `extra` widens every row, so that two buffers of one
    picture can have different strides"""

    def __init__(self, torch, planes, bd, extra=0):
        self.bd, self.extra, self.host, self.dev, self.ptr, self.stride = bd, extra, [], [], [], []
        for p, pl in enumerate(planes):
            ph, pw = pl.shape
            big = np.full((ph + 2 * GUARD, pw + 2 * GUARD + p + extra), FILL[bd] + p, pl.dtype)
            big[GUARD:GUARD + ph, GUARD:GUARD + pw] = pl
            d = _dev(torch, big)
            self.host.append(big), self.dev.append(d)
            self.ptr.append(d.data_ptr() + (GUARD * big.shape[1] + GUARD) * big.itemsize)
            self.stride.append(big.shape[1])

    def planes(self):
        """(planes, guard untouched)"""
        out, ok = [], True
        for p in range(3):
            big = self.dev[p].cpu().numpy().view(self.host[p].dtype).reshape(self.host[p].shape)
            ph, pw = big.shape[0] - 2 * GUARD, big.shape[1] - 2 * GUARD - p - self.extra
            out.append(big[GUARD:GUARD + ph, GUARD:GUARD + pw].copy())
            mask = np.ones(big.shape, bool)
            mask[GUARD:GUARD + ph, GUARD:GUARD + pw] = False
            ok &= bool(np.all(big[mask] == FILL[self.bd] + p))
        return out, ok


class DevCase:
    """a fixture case on the device: guarded planes, the picture, and a zeroed workspace of work_bytes"""

    def __init__(self, torch, F, work_bytes):
        self.F, self.bd = F, F["bd"]
        self.cdef, self.dbk, self.src = (Guarded(torch, F[k], F["bd"]) for k in ("cdef", "dbk", "src"))
        self.out = Guarded(torch, [np.full_like(p, 7) for p in F["cdef"]], F["bd"])
        self.pic = svtav1_hip.make_lr_picture(F["w"], F["h"], self.cdef.ptr, self.cdef.stride, self.dbk.ptr, self.dbk.stride, self.src.ptr,
                                              self.src.stride)
        self.n = F["base"][3]
        self.work = torch.zeros(work_bytes // 8 + 1, dtype=torch.int64, device="cuda:0")
        _ready(torch)

    def inputs_untouched(self):
        return all(g.planes()[1] and all(np.array_equal(a, b) for a, b in zip(g.planes()[0], self.F[k]))
                   for g, k in ((self.cdef, "cdef"), (self.dbk, "dbk"), (self.src, "src")))
