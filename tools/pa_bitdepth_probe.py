#!/usr/bin/env python3
"""Times the five entries of the 10-bit picture forms on 12 pictures of 1920 x 1080 per launch and on one picture of 3840 x 2160:
svthip_pa_unpack_10bit_dev with and without the 2-bit planes, svthip_pa_pack_10bit_dev, svthip_pa_pack_10bit_compressed_dev,
svthip_picture_sse_dev and svthip_highbd_picture_sse_dev in its three source forms (each SSE call is its partial-sum launch plus its finish).
Next to every entry, in the same run: a device-to-device copy of a buffer of as many bytes as the entry reads plus writes (the yardstick of
DESIGN 3.5; that copy moves every one of those bytes twice) and a copy of half that buffer (the same traffic as the entry).  For ingest and
SSE also the host transfer the entry removes: the upload of the 8-bit interiors a host-side unpack would have to send, and the download of
the reconstructed 16-bit planes a host-side PSNR would have to fetch (pageable host memory, host clock around synchronous copies).

    python tools/pa_bitdepth_probe.py [--iters N] [--out FILE]          device times (needs a GPU)
    python tools/pa_bitdepth_probe.py --resources FILE                  registers, LDS and scratch of the kernels from the compiler's remarks

Device times are microseconds per LAUNCH: the median over N samples, each the mean of back-to-back calls queued behind a sleep kernel, as
tools/probe_common.py: timed takes them.  Planes are tight (stride = width), so every row starts 16-byte aligned; bytes are what the algorithm
reads and writes, computed from the shapes, and GB/s is bytes over the time.  One JSON line per row, appended to --out."""
import argparse

import numpy as np

from probe_common import add_common_args, emit, host_timed, open_stream, resources, timed, write_rows  # sets the import path

SHAPES = ((1920, 1080, 12), (3840, 2160, 1))   # width, height, pictures per launch


def device_times(lines, iters):
    import torch

    import bitdepth_util as bu
    import svtav1_hip
    ctx = svtav1_hip.Context(0)
    _, stream = open_stream(torch)

    def host_copy(name, dst, src, n, nbytes, **more):
        us = host_timed(lambda: (dst.copy_(src), torch.cuda.synchronize()), iters, torch.cuda.synchronize).median
        emit(lines, {"entry": name, "kind": "host clock around synchronous copies", "width": w, "height": h, "pictures": n, "us": round(us, 1), "bytes": nbytes,
                     "GB_per_s": round(nbytes / us / 1e3, 1), **more})

    for w, h, n in SHAPES:
        rng = np.random.default_rng(w)
        dims = bu.plane_dims(w, h)
        P = w * h * 3 // 2          # samples of a picture

        def tight(dtype, fill):
            """n pictures' tight planes in one flat device array: (tensor, [svthip_planes])"""
            offs, at = [], 0
            for _ in range(n):
                o = []
                for ph, pw in dims:
                    o.append(at)
                    at += ph * pw
                offs.append(o)
            host = fill(at).astype(dtype)
            return torch.from_numpy(host.view(np.uint8)).to("cuda:0"), [svtav1_hip.make_planes(o, [w, w // 2, w // 2]) for o in offs], host, offs

        d_in16, p16, h_in16, offs = tight(np.uint16, lambda k: rng.integers(0, 1024, k))
        d_out8, p8, _, _ = tight(np.uint8, lambda k: np.zeros(k))
        d_outn, pn, _, _ = tight(np.uint8, lambda k: np.zeros(k))
        d_back, pb, _, _ = tight(np.uint16, lambda k: np.zeros(k))
        d_recon16, pr16, h_recon16, _ = tight(np.uint16, lambda k: rng.integers(0, 1024, k))
        d_recon8, pr8, h_recon8, _ = tight(np.uint8, lambda k: rng.integers(0, 256, k))
        h_tiled = rng.integers(0, 256, n * P // 4).astype(np.uint8)
        d_tiled = torch.from_numpy(h_tiled).to("cuda:0")
        pt, at = [], 0
        for _ in range(n):
            o = []
            for ph, pw in dims:
                o.append(at)
                at += ph * pw // 4
            pt.append(svtav1_hip.make_planes(o, [0, 0, 0]))
        d_sse = torch.zeros((4, n, 3), dtype=torch.int64, device="cuda:0")
        sse_at = lambda k: d_sse.data_ptr() + k * n * 24  # noqa: E731
        A = lambda t: t.data_ptr()  # noqa: E731
        entries = [
            ("pa_unpack_10bit (8-bit and 2-bit planes)", 4 * P, lambda: ctx.pa_unpack_10bit_dev(A(d_in16), p16, A(d_out8), p8, A(d_outn), pn, w, h, stream=stream)),
            ("pa_unpack_10bit (8-bit planes alone)", 3 * P, lambda: ctx.pa_unpack_10bit_dev(A(d_in16), p16, A(d_out8), p8, None, None, w, h, stream=stream)),
            ("pa_pack_10bit", 4 * P, lambda: ctx.pa_pack_10bit_dev(A(d_out8), p8, A(d_outn), pn, A(d_back), pb, w, h, stream=stream)),
            ("pa_pack_10bit_compressed", 3 * P + P // 4, lambda: ctx.pa_pack_10bit_dev(A(d_out8), p8, A(d_tiled), pt, A(d_back), pb, w, h, compressed=True,
                                                                                      stream=stream)),
            ("picture_sse (8-bit)", 2 * P, lambda: ctx.picture_sse_dev(A(d_recon8), pr8, A(d_out8), p8, w, h, sse_at(0), stream=stream)),
            ("highbd_picture_sse (16-bit source)", 4 * P, lambda: ctx.highbd_picture_sse_dev(A(d_recon16), pr16, svtav1_hip.SSE_SRC_16BIT, A(d_in16), p16, None,
                                                                                             None, w, h, sse_at(1), stream=stream)),
            ("highbd_picture_sse (8-bit + unpacked 2-bit source)", 4 * P, lambda: ctx.highbd_picture_sse_dev(
                A(d_recon16), pr16, svtav1_hip.SSE_SRC_UNPACKED, A(d_out8), p8, A(d_outn), pn, w, h, sse_at(2), stream=stream)),
            ("highbd_picture_sse (8-bit + compressed 2-bit source)", 3 * P + P // 4, lambda: ctx.highbd_picture_sse_dev(
                A(d_recon16), pr16, svtav1_hip.SSE_SRC_COMPRESSED, A(d_out8), p8, A(d_tiled), pt, w, h, sse_at(3), stream=stream)),
        ]
        torch.cuda.synchronize()
        copies = {}
        for name, per_pic, fn in entries:
            nbytes = n * per_pic
            us = timed(torch, fn, iters, 10).median
            if nbytes not in copies:
                src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
                dst = torch.zeros_like(src)
                copies[nbytes] = (timed(torch, lambda: dst.copy_(src), iters, 10).median,
                                  timed(torch, lambda: dst[:nbytes // 2].copy_(src[:nbytes // 2]), iters, 10).median)
                del src, dst
            copy_us, half_us = copies[nbytes]
            row = {"entry": name, "kind": "device events", "width": w, "height": h, "pictures": n, "us": round(us, 1), "bytes": nbytes,
                   "GB_per_s": round(nbytes / us / 1e3, 1), "copy_of_as_many_bytes_us": round(copy_us, 1), "ratio_to_that_copy": round(us / copy_us, 2),
                   "copy_of_the_same_traffic_us": round(half_us, 1), "ratio_to_the_same_traffic": round(us / half_us, 2)}
            emit(lines, row)
        # correctness of what was timed, on the first and the last picture
        torch.cuda.synchronize()
        out8, outn = d_out8.cpu().numpy(), d_outn.cpu().numpy()
        back = d_back.cpu().numpy().view(np.uint16)
        sums = d_sse.cpu().numpy().view(np.uint64)
        for j in (0, n - 1):
            for pl, (ph, pw) in enumerate(dims):
                o = offs[j][pl]
                a = h_in16[o:o + ph * pw].reshape(ph, pw)
                w8, wn = bu.unpack(a)
                assert np.array_equal(out8[o:o + ph * pw].reshape(ph, pw), w8) and np.array_equal(outn[o:o + ph * pw].reshape(ph, pw), wn), "timed unpack differs"
                to = sum(x * y // 4 for x, y in dims) * j + sum(x * y // 4 for x, y in dims[:pl])
                wc = bu.pack_compressed(w8, h_tiled[to:to + ph * pw // 4], bu.sb_size(pl))
                assert np.array_equal(back[o:o + ph * pw].reshape(ph, pw), wc), "timed compressed pack differs"   # the last of the two packs that ran
                r16, r8 = h_recon16[o:o + ph * pw].reshape(ph, pw), h_recon8[o:o + ph * pw].reshape(ph, pw)
                want = [bu.sse(r8, w8), bu.sse(r16, a), bu.sse(r16, bu.pack(w8, wn)), bu.sse(r16, wc)]
                assert [int(sums[k, j, pl]) for k in range(4)] == [int(v) for v in want], "timed picture SSE differs"
        # the host transfers the entries remove
        unpack_us = next(r["us"] for r in lines if r["entry"].startswith("pa_unpack_10bit (8-bit and") and r["width"] == w)
        sse_us = next(r["us"] for r in lines if r["entry"].startswith("highbd_picture_sse (8-bit + unpacked") and r["width"] == w)
        host8 = torch.zeros(n * P, dtype=torch.uint8)
        host_copy(f"yardstick: upload of the 8-bit interiors of {n} picture(s) from pageable host memory (what a host-side unpack has to send)", d_out8, host8,
                  n, n * P, unpack_with_2bit_us=unpack_us, cheaper_than_the_upload=None)
        lines[-1]["cheaper_than_the_upload"] = unpack_us < lines[-1]["us"]
        host16 = torch.zeros(2 * n * P, dtype=torch.uint8)
        host_copy(f"yardstick: download of the reconstructed 16-bit planes of {n} picture(s) to pageable host memory (what a host-side PSNR has to fetch)",
                  host16, d_recon16, n, 2 * n * P, highbd_sse_unpacked_us=sse_us, cheaper_than_the_download=None)
        lines[-1]["cheaper_than_the_download"] = sse_us < lines[-1]["us"]
        del d_in16, d_out8, d_outn, d_back, d_recon16, d_recon8, d_tiled
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap, 7, resources=True)
    a = ap.parse_args()
    lines = []
    if a.resources:
        return resources("pa_bitdepth.hip", a.resources)
    device_times(lines, a.iters)
    write_rows(a.out, lines)


if __name__ == "__main__":
    main()
