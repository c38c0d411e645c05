#!/usr/bin/env python3
"""Device time of resize (pixo_hip_resize_device: the product's kernels, no PCIe) against a plain copy of the same bytes in
the same run, and the reference's wasm on the host where node and oracle/_ref/ are present.

Shapes: 4096x4096 -> 1024x1024, 1920x1080 -> 640x360, 1024x1024 -> 4096x4096; Rgb and Rgba; nearest, bilinear, Lanczos3.
Every timed call uses the next of a ring of source/destination pairs whose total exceeds the 256 MiB Infinity Cache, so the
bytes come from HBM.  HIP events around blocks of calls; median and minimum of 7 blocks after a warm-up of every pair.
The copy is pixo_hip_debug_stream_copy over source + destination bytes (rounded up to its 24 KiB granule) on the same ring:
a resize's memory floor is its source plus its destination (plus twice the intermediate for Lanczos3, reported beside it).

    python tools/resize_timing.py [--out profiles/resize_timing.txt] [--no-wasm]
"""
import argparse
import ctypes as C
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import resize_cases as RC  # noqa: E402
import synth  # noqa: E402
from pixo_amd import ColorType, _lib, resize  # noqa: E402

SHAPES = [(4096, 4096, 1024, 1024), (1920, 1080, 640, 360), (1024, 1024, 4096, 4096)]
RING_BYTES = 320 << 20
GRANULE = 24576


def timed(fn, ring, blocks=7):
    for i in range(ring):  # warm-up: every pair once
        fn(i)
    torch.cuda.synchronize()
    per = max(ring, 20)
    us = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(per):
            fn(i % ring)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / per * 1e3)
    return statistics.median(us), min(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-wasm", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resize_timing.py measures on the GPU; there is no CPU fallback"
    L = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    lines = ["resize device time, %s on %s (%s)" % (L.pixo_hip_version().decode(), torch.cuda.get_device_name(0), socket.gethostname()),
             "ring of source/destination pairs > %d MiB; median (min) of 7 blocks, HIP events; copy = pixo_hip_debug_stream_copy of src + dst bytes" % (RING_BYTES >> 20),
             "%-22s %-5s %-9s %12s %12s %8s %10s %12s" % ("shape", "ct", "algorithm", "resize us", "copy us", "x copy", "GB/s", "wasm ms")]
    for (sw, sh, dw, dh) in SHAPES:
        for ct in (2, 3):
            bpp = RC.BPP[ct]
            n_in, n_out = sw * sh * bpp, dw * dh * bpp
            moved = n_in + n_out
            copy_bytes = (moved + GRANULE - 1) // GRANULE * GRANULE
            ring = RING_BYTES // (2 * copy_bytes) + 2  # (every pair: copy_bytes in, copy_bytes out)
            px = synth.lcg_bytes(n_in, 5)
            srcs = [torch.zeros(copy_bytes, dtype=torch.uint8, device="cuda:0") for _ in range(ring)]
            dsts = [torch.zeros(copy_bytes, dtype=torch.uint8, device="cuda:0") for _ in range(ring)]
            h = torch.from_numpy(px)
            for s in srcs:
                s[:n_in] = h.to("cuda:0")
            torch.cuda.synchronize()

            def copy(i):
                rc = L.pixo_hip_debug_stream_copy(srcs[i].data_ptr(), dsts[i].data_ptr(), copy_bytes, C.c_void_p(stream) if stream else None)
                assert rc == 0, L.pixo_hip_last_error()

            copy_us, copy_min = timed(copy, ring)
            for algo in (0, 1, 2):
                o = resize.ResizeOptions.builder(sw, sh).dst(dw, dh).color_type(ColorType(ct)).algorithm(resize.ResizeAlgorithm(algo)).build()

                def run(i):
                    resize.resize_device(srcs[i], o, dsts[i], stream)

                us, mn = timed(run, ring)
                wasm = "-"
                if not a.no_wasm and RC.have_live_wasm():
                    c = dict(sw=sw, sh=sh, dw=dw, dh=dh, color_type=ct, algorithm=algo)
                    (data, err, ms), = RC.run_wasm([c], [px], repeat=3)
                    assert err is None, err
                    got = dsts[(max(ring, 20) - 1) % ring][:n_out].cpu().numpy().tobytes()
                    assert got == data, "device output differs from the wasm's: %s" % RC.first_difference(got, data)
                    wasm = "%.1f" % min(ms)
                extra = "" if algo != 2 else "  (+ intermediate %d MB written and read)" % (dw * sh * bpp // 1000000)
                lines.append("%-22s %-5s %-9s %7.1f (%5.1f) %6.1f (%5.1f) %8.2f %10.0f %12s%s" % (
                    "%dx%d->%dx%d" % (sw, sh, dw, dh), ColorType(ct).name, RC.ALGO_NAMES[algo], us, mn, copy_us, copy_min, us / copy_us,
                    moved / us / 1e3, wasm, extra))
                print(lines[-1], flush=True)
            del srcs, dsts
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
