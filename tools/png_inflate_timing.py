#!/usr/bin/env python3
"""The PNG decode batch with the inflates on the device (PIXO_DECODE_DEVICE_INFLATE: one wavefront per stream, all streams of a
sub-batch in one launch) against the same call without the flag — the host inflate on 8 threads, and on the calling thread
(one_thread) —, on the same build in the same run.

Workloads: 64 files of 1920x1080 in the three contents of tools/png_decode_batch_timing.py (every row Paeth, the adaptive
filters of our own encoder, 8-bit palette; eight distinct images per content), and 1024 files of 256x256 of the adaptive content:
the shape where the streams outnumber the host's threads by far.  Per workload: wall time of the device entry up to the
synchronisation of its stream for the three forms, median and minimum of ROUNDS rounds after WARMUP warm-up rounds, the forms
alternating; and the inflate launch alone (pixo_hip_debug_zlib_inflate_batch_device: HIP events around the launch), with the rate
at which ONE stream is inflated (its output bytes over the launch time: every stream has a wavefront of its own, so the launch
takes as long as its slowest stream) and the rate of the launch as a whole.  Before timing, the images with the flag are compared
with those without, and the route record is read: bit 44 would say that the host inflated a stream again.

    python tools/png_inflate_timing.py [--out profiles/png_inflate_timing.txt]
"""
import argparse
import os
import socket
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import png_decode_cases as PC  # noqa: E402
import png_decode_model as M  # noqa: E402
import png_file_cases as FC  # noqa: E402
import synth  # noqa: E402
from pixo_amd import ColorType, _lib, decode, jpeg, png  # noqa: E402

DISTINCT = 8
WARMUP, ROUNDS = 2, 7


def paeth_file(px, w, h):
    stream = PC.filter_rows(px.tobytes(), h, w * 3, 3, [4] * h)
    return M.SIGNATURE + PC.chunk(b"IHDR", PC.ihdr(w, h, 8, PC.RGB)) + PC.chunk(b"IDAT", zlib.compress(stream, 6)) + PC.chunk(b"IEND", b"")


def adaptive(w, h, seed):
    o = png.PngOptions.builder(w, h).color_type(ColorType.Rgb).preset(1).flags(png.NO_RAYON).build()
    return [png.encode(synth.scene(w, h, seed + k), o) for k in range(DISTINCT)]


def workloads():
    W, H = 1920, 1080
    yield "all-Paeth scene", W, H, 64, [paeth_file(synth.scene(W, H, 300 + k), W, H) for k in range(DISTINCT)]
    yield "adaptive scene (our encoder)", W, H, 64, adaptive(W, H, 300)
    yield "palette, 8 bits", W, H, 64, [PC.make(W, H, PC.INDEXED, 8, seed=400 + k) for k in range(DISTINCT)]
    yield "adaptive scene (our encoder)", 256, 256, 1024, adaptive(256, 256, 500)


def med(v):
    return statistics.median(v), min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_inflate_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "png_inflate_timing.py measures on the GPU; there is no CPU fallback"
    L = _lib.load()
    lines = ["PNG decode batch: inflate on the device against inflate on the host, %s on %s (%s)" % (
                 L.pixo_hip_version().decode(), torch.cuda.get_device_name(0), socket.gethostname()),
             "ms, median (min) of %d rounds after %d warm-up rounds, the forms alternating; call = wall time of the device entry up to the" % (ROUNDS, WARMUP),
             "synchronisation of its stream; inflate launch = HIP events around the one launch that inflates every stream of the batch"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for kind, w, h, n, distinct in workloads():
        files = [distinct[i % DISTINCT] for i in range(n)]
        _, total = decode.decode_png_batch_info(files)
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        ref = torch.empty(total, dtype=torch.uint8, device="cuda")
        decode.decode_png_batch_device(files, out=ref)
        jpeg.debug_routes(clear=True)
        decode.decode_png_batch_device(files, out=out, device_inflate=True)
        torch.cuda.synchronize()
        bits = jpeg.debug_routes(clear=True)
        same = torch.equal(out, ref)
        redo = bool(bits >> decode.INFLATE_ROUTES["PNG_INFLATE_HOST_REDO"] & 1)

        def call(**kw):
            t0 = time.perf_counter()
            decode.decode_png_batch_device(files, out=out, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        streams = [b"".join(FC.parse(f)[0]) for f in distinct]
        sizes = [len(zlib.decompress(z)) for z in streams]
        streams, sizes = [streams[i % DISTINCT] for i in range(n)], [sizes[i % DISTINCT] for i in range(n)]
        at, out_at = 0, []
        for s in sizes:
            out_at.append(at)
            at += (s + 15) // 16 * 16
        block = np.zeros(at, np.uint8)

        def launch():
            verdicts, _, _, ms = decode.inflate_zlib_batch_debug(streams, sizes, block, out_at)
            assert not any(verdicts), verdicts
            return ms

        forms = {"device inflate": dict(device_inflate=True), "host, 8 threads": dict(), "host, one_thread": dict(one_thread=True)}
        calls, kernel = {k: [] for k in forms}, []
        for r in range(WARMUP + ROUNDS):
            got = {k: call(**kw) for k, kw in forms.items()}
            ms = launch()
            if r >= WARMUP:
                kernel.append(ms)
                for k in forms:
                    calls[k].append(got[k])
        lines.append("")
        lines.append("%s, %d files of %dx%d: %.1f MiB of files, %.1f MiB of inflated streams%s%s" % (
            kind, n, w, h, sum(len(f) for f in files) / 2**20, sum(sizes) / 2**20, "" if same else "   OUTPUTS DIFFER",
            "   THE HOST INFLATED A STREAM AGAIN" if redo else ""))
        for k in forms:
            lines.append("  %-18s %9.2f (%8.2f) ms a call" % ((k,) + med(calls[k])))
        km, klo = med(kernel)
        lines.append("  %-18s %9.2f (%8.2f) ms: one stream at %.1f MB/s of output (the largest, %.2f MB), the launch at %.0f MB/s" % (
            "inflate launch", km, klo, max(sizes) / 1e3 / km, max(sizes) / 1e6, sum(sizes) / 1e3 / km))
        lines.append("  device inflate / host, 8 threads: %.2f; device inflate / host, one_thread: %.2f (call time; below 1: the device path is faster)" % (
            med(calls["device inflate"])[0] / med(calls["host, 8 threads"])[0], med(calls["device inflate"])[0] / med(calls["host, one_thread"])[0]))
        print("\n".join(lines[-7:]), flush=True)
        with open(a.out, "w") as f:  # (kept current: a later workload may run out of time)
            f.write("\n".join(lines) + "\n")
        del out, ref
    print("wrote", a.out)


if __name__ == "__main__":
    main()
