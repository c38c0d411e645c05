#!/usr/bin/env python3
"""A PNG decode batch (pixo_hip_png_decode_batch_device: the inflates on a pool of host threads, one upload, one launch per
pass for all files) against a loop of pixo_hip_png_decode_device calls over the same files, on the same build in the same run.

Workload: 64 files of 1920x1080 in three contents — every row Paeth (a scene; each file is ONE run of rows, the case the
no-waiting rule of DESIGN.md §4.6e pays most for), the adaptive filters of our own encoder on the same scenes, and 8-bit
palette files.  Eight distinct images per content, each eight times in the list (the host work per entry is the same; it
keeps the making of the files short).  Per content: wall time of the call up to the stream's synchronisation for the batch
(threaded and with one_thread) and for the loop, median and minimum of ROUNDS rounds after WARMUP warm-up rounds, the three
forms alternating; and the legs — inflate (host clock), upload, unfilter, convert (HIP events) — from the timed debug entries
(pixo_hip_debug_png_decode_batch_timed; pixo_hip_debug_png_decode_timed summed over the files), median of the same rounds.
Before timing, the batch's images are compared with the loop's.

    python tools/png_decode_batch_timing.py [--out profiles/png_decode_batch_timing.txt] [--files 64]
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

import png_decode_cases as PC  # noqa: E402
import png_decode_model as M  # noqa: E402
import synth  # noqa: E402
from pixo_amd import ColorType, _lib, decode, png  # noqa: E402

W, H = 1920, 1080
DISTINCT = 8
WARMUP, ROUNDS = 2, 7


def paeth_file(px):
    stream = PC.filter_rows(px.tobytes(), H, W * 3, 3, [4] * H)
    return M.SIGNATURE + PC.chunk(b"IHDR", PC.ihdr(W, H, 8, PC.RGB)) + PC.chunk(b"IDAT", zlib.compress(stream, 6)) + PC.chunk(b"IEND", b"")


def contents(n):
    scenes = [synth.scene(W, H, 300 + k) for k in range(DISTINCT)]
    o = png.PngOptions.builder(W, H).color_type(ColorType.Rgb).preset(1).flags(png.NO_RAYON).build()
    kinds = {
        "all-Paeth scene": [paeth_file(s) for s in scenes],
        "adaptive scene (our encoder)": [png.encode(s, o) for s in scenes],
        "palette, 8 bits": [PC.make(W, H, PC.INDEXED, 8, seed=400 + k) for k in range(DISTINCT)],
    }
    return {k: [v[i % DISTINCT] for i in range(n)] for k, v in kinds.items()}


def med(v):
    return statistics.median(v), min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode_batch_timing.txt"))
    ap.add_argument("--files", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "png_decode_batch_timing.py measures on the GPU; there is no CPU fallback"
    L = _lib.load()
    n = a.files
    lines = ["PNG decode batch against a loop of single calls, %s on %s (%s)" % (L.pixo_hip_version().decode(), torch.cuda.get_device_name(0), socket.gethostname()),
             "%d files of %dx%d (%d distinct per content); ms, median (min) of %d rounds after %d warm-up rounds, the forms alternating;" % (n, W, H, DISTINCT, ROUNDS, WARMUP),
             "call = wall time of the device entry up to the synchronisation of its stream; legs: inflate on the host clock, the rest HIP events",
             "(the timed entries copy the pixels to the host as well: their legs are not the call column's parts to the microsecond)"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for kind, files in contents(n).items():
        arr, held = decode._files_c(files)
        _, total = decode.decode_png_batch_info(files)
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        each = torch.empty(W * H * 4, dtype=torch.uint8, device="cuda")
        # the same pixels from both forms
        views = decode.decode_png_batch_device(files, out=out)
        same = all(torch.equal(t, decode.decode_png_device(f)[0]) for (t, _), f in zip(views[:DISTINCT], files[:DISTINCT]))
        torch.cuda.synchronize()

        def batch(one_thread):
            t0 = time.perf_counter()
            decode.decode_png_batch_device(files, out=out, one_thread=one_thread)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def loop():
            t0 = time.perf_counter()
            for f in held:
                decode.decode_png_device(f, out=each)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def batch_legs(flags):
            ms = (C.c_double * 5)()
            rc = L.pixo_hip_debug_png_decode_batch_timed(arr, n, flags, ms)
            assert rc == 0, L.pixo_hip_last_error()
            return list(ms)

        def loop_legs():
            legs = [0.0] * 5
            ms, counts = (C.c_double * 7)(), (C.c_uint64 * 3)()
            t0 = time.perf_counter()
            for f in held:
                rc = L.pixo_hip_debug_png_decode_timed(f.ctypes.data, f.size, ms, counts)
                assert rc == 0, L.pixo_hip_last_error()
                for k, v in enumerate((ms[1] + ms[2], ms[3], ms[4], ms[5])):
                    legs[k] += v
            legs[4] = (time.perf_counter() - t0) * 1e3
            return legs

        calls = {"batch": [], "batch one_thread": [], "loop": []}
        legs = {"batch": [], "batch one_thread": [], "loop": []}
        for r in range(WARMUP + ROUNDS):
            got = {"batch": batch(False), "batch one_thread": batch(True), "loop": loop()}
            got_legs = {"batch": batch_legs(0), "batch one_thread": batch_legs(decode.ONE_THREAD), "loop": loop_legs()}
            if r >= WARMUP:
                for k in calls:
                    calls[k].append(got[k])
                    legs[k].append(got_legs[k])
        plan = decode.decode_png_batch_plan(files)
        lines.append("")
        lines.append("%s: %.1f MiB of files, %.1f MiB of pixels, %d runs of rows in %d unfilter + %d convert launches, %d inflate threads%s" % (
            kind, sum(len(f) for f in files) / 2**20, total / 2**20, sum(plan["runs"]), plan["unfilter_launches"], plan["convert_launches"],
            plan["threads"], "" if same else "   OUTPUTS DIFFER"))
        lines.append("  %-18s %19s | %9s %9s %9s %9s %11s" % ("form", "call ms", "inflate", "upload", "unfilter", "convert", "timed call"))
        for k in calls:
            m, lo = med(calls[k])
            leg = [statistics.median(x[i] for x in legs[k]) for i in range(5)]
            lines.append("  %-18s %9.2f (%7.2f) | %9.2f %9.2f %9.2f %9.2f %11.2f" % (k, m, lo, *leg))
        lines.append("  loop / batch: %.2f (call), %.2f (unfilter leg); batch one_thread / batch: %.2f (call)" % (
            med(calls["loop"])[0] / med(calls["batch"])[0],
            statistics.median(x[2] for x in legs["loop"]) / max(statistics.median(x[2] for x in legs["batch"]), 1e-9),
            med(calls["batch one_thread"])[0] / med(calls["batch"])[0]))
        print("\n".join(lines[-6:]), flush=True)
        with open(a.out, "w") as f:  # (kept current: a later content may run out of time)
            f.write("\n".join(lines) + "\n")
        del out, each
    print("wrote", a.out)


if __name__ == "__main__":
    main()
