#!/usr/bin/env python3
"""Where the time of a PNG decode goes (pixo_hip_debug_png_decode_timed: the product's call with its legs timed), for
4096x4096 RGBA and RGB files written by the library's own encoder from synth.scene and from noise, with the encoder's adaptive
filters and with Paeth on every row (one segment: the reconstruction kernel's worst case).

Legs: chunk walk + CRC, inflate, finding the runs (host clocks); upload, reconstruction kernel, conversion kernel (HIP events);
the whole call.  Beside the conversion kernel a plain copy of the same bytes in the same run (pixo_hip_debug_stream_copy over
rows + pixels, rounded up to its 24 KiB granule).  Beside the reconstruction kernel the baseline: a plain single-thread C++ loop
over the same inflated stream, compiled from the same arithmetic header (tests/emu_png_unfilter/), timed in this script.
One warm-up call per file, then the median (minimum) of 5 calls; the loop: median of 3.

    python tools/png_decode_timing.py [--out profiles/png_decode_timing.txt] [--size 4096]
"""
import argparse
import ctypes as C
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

import emu_png_unfilter_lib as E  # noqa: E402
import png_decode_model as M  # noqa: E402
import synth  # noqa: E402
from pixo_amd import ColorType, _lib, decode, png  # noqa: E402

GRANULE = 24576
LEGS = ["walk+crc", "inflate", "runs", "upload", "unfilter", "convert", "whole"]


def host_loop_ms(stream, h, rb, bpp, reps=3):
    L = E.lib()
    s = np.frombuffer(stream, np.uint8)
    rows = np.zeros(h * rb, np.uint8)
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        assert L.emu_pngu_unfilter(s.ctypes.data, h, rb, bpp, rows.ctypes.data) == -1
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), rows


def copy_us(L, nbytes, stream):
    n = (nbytes + GRANULE - 1) // GRANULE * GRANULE
    a, b = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    us = []
    for i in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        assert L.pixo_hip_debug_stream_copy(a.data_ptr(), b.data_ptr(), n, C.c_void_p(stream) if stream else None) == 0
        e1.record()
        torch.cuda.synchronize()
        if i:
            us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "png_decode_timing.py measures on the GPU; there is no CPU fallback"
    L = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    n = a.size
    lines = ["PNG decode legs, %s on %s (%s)" % (L.pixo_hip_version().decode(), torch.cuda.get_device_name(0), socket.gethostname()),
             "%dx%d files from the library's own encoder; 1 warm-up, median (min) of 5 calls in ms; copy: pixo_hip_debug_stream_copy of rows + pixels; "
             "host loop: one thread, tests/emu_png_unfilter (png_unfilter_math.h), median of 3" % (n, n),
             "%-22s %9s | %s | %10s %10s %8s | %11s %8s" % ("file", "file MB", " ".join("%14s" % s for s in LEGS), "segments", "longest", "groups",
                                                         "host loop ms", "x kernel")]
    ratios = {}
    made = {"scene": np.asarray(synth.scene(n, n, 5), np.uint8).reshape(n * n, 3), "noise": np.asarray(synth.noise(n, n, 5), np.uint8).reshape(n * n, 3)}
    for ct, ch in ((ColorType.Rgba, 4), (ColorType.Rgb, 3)):
        for content in ("scene", "noise"):
            rgb = made[content]
            px = rgb if ch == 3 else np.concatenate([rgb, (255 - rgb[:, 1:2] // 4).astype(np.uint8)], axis=1)
            for strategy in (png.FilterStrategy.ADAPTIVE, png.FilterStrategy.PAETH):
                o = png.PngOptions.builder(n, n).color_type(ct).preset(0).reduce_color_type(False).reduce_palette(False).optimize_alpha(False) \
                    .filter_strategy(strategy).flags(png.NO_RAYON).build()
                file = png.encode(px, o)
                f = np.frombuffer(file, np.uint8)
                ms, counts = (C.c_double * 7)(), (C.c_uint64 * 3)()
                runs = []
                for i in range(6):
                    rc = L.pixo_hip_debug_png_decode_timed(f.ctypes.data, f.size, ms, counts)
                    assert rc == 0, L.pixo_hip_last_error()
                    if i:
                        runs.append(list(ms))
                im = decode.decode_png(file)
                assert im.pixels == px.tobytes(), "decoded pixels differ from the encoder's input"
                med = [statistics.median(r[k] for r in runs) for k in range(7)]
                mn = [min(r[k] for r in runs) for k in range(7)]
                w = M.walk(file)
                rb = M.row_bytes(w["color_type"], w["depth"], n)
                loop_ms, _ = host_loop_ms(zlib.decompress(w["idat"]), n, rb, M.filter_unit(w["color_type"], w["depth"]))
                name = "%s %s %s" % (ct.name, content, strategy.name.lower())
                ratios[name] = loop_ms / med[4]
                lines.append("%-22s %9.1f | %s | %10d %10d %8d | %11.1f %8.2f" % (
                    name, len(file) / 1e6, " ".join("%7.2f (%5.2f)" % (med[k], mn[k]) for k in range(7)), counts[0], counts[1], counts[2],
                    loop_ms, loop_ms / med[4]))
                print(lines[-1], flush=True)
            cu = copy_us(L, n * ((n * ch + 15) // 16 * 16) + n * n * ch, stream)
            lines.append("%-22s conversion's bytes (rows + pixels) by a plain copy in the same run: %.3f ms" % ("%s %s" % (ct.name, content), cu / 1e3))
    lines.append("x kernel = host loop / reconstruction kernel.  Worst case (Paeth on every row, one segment, one wavefront): " +
                 "; ".join("%s %.2f (%s wins)" % (k, v, "the kernel" if v > 1 else "the host loop") for k, v in ratios.items() if k.endswith("paeth")))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
