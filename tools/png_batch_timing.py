#!/usr/bin/env python3
"""PNG batches against a loop of single calls over the same resident images.

    python tools/png_batch_timing.py            -> profiles/png_batch_timing.txt

Shapes: 64 x 256^2 RGB, 1024 x 64^2 RGB, 64 x 1920x1080 RGB; preset 0 on each, preset 1 as well on the 256^2 shape; content:
photo-like (`synth.scene`) and noise.  `png.encode_batch_device` against a loop of `png.encode_device` over the same
images in HBM — both end in the same DEFLATE tail, the loop with a table of one segment per call.  Batch and loop alternate, every shape is warmed up
first.  Written: host wall time around the call (median [min .. max] over the repeats), files per second, the spread, and
for the batch the wall time between the host's waits as the library's `trace` switch prints it (one more call per row, its
stderr captured; these are host times around device work, not device events).  Where the batch does not win, the row says so.
"""
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(64, 256, 256, (0, 1)), (1024, 64, 64, (0,)), (64, 1920, 1080, (0,))]
REPEATS = 7


def images(kind, n, w, h):
    import synth
    distinct = min(n, 8)  # (content generation is host time: eight different images, repeated)
    base = [synth.scene(w, h, 100 + i) if kind == "photo" else synth.lcg_bytes(w * h * 3, 200 + i) for i in range(distinct)]
    return [base[i % distinct] for i in range(n)]


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def traced(fn):
    """one call with the trace switch on: the library's '[pixo_hip] png batch' lines"""
    from pixo_amd import _lib
    L = _lib.load()
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        L.pixo_hip_debug_configure(b"trace")
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            L.pixo_hip_debug_configure(None)
        tmp.seek(0)
        return [ln.strip() for ln in tmp.read().decode(errors="replace").splitlines() if "png batch" in ln]


def main():
    import torch
    from pixo_amd import ColorType, png
    path = os.path.join(ROOT, "profiles", "png_batch_timing.txt")
    lines = ["# png.encode_batch_device against a loop of png.encode_device over the same images in HBM; host wall time around the",
             "# call in ms, median [min .. max] of %d alternating repeats after a warm-up of both; spread = (max - min) / median" % REPEATS,
             "# device: %s" % torch.cuda.get_device_name(0), ""]
    for n, w, h, presets in SHAPES:
        for preset in presets:
            for kind in ("photo", "noise"):
                px = images(kind, n, w, h)
                d_all = torch.from_numpy(np.concatenate(px)).cuda()
                d_one = [d_all[i * w * h * 3:(i + 1) * w * h * 3] for i in range(n)]
                o = png.PngOptions.builder(w, h).color_type(ColorType.Rgb).preset(preset).build()
                batch = lambda: png.encode_batch_device(d_all, o, n)
                loop = lambda: [png.encode_device(d, o) for d in d_one]
                same = batch() == loop()  # (the warm-up of both)
                tb, tl = [], []
                for _ in range(REPEATS):
                    tb.append(wall(batch)[0])
                    tl.append(wall(loop)[0])
                mb, ml = statistics.median(tb), statistics.median(tl)
                row = "%4d x %4dx%-4d RGB preset %d %-5s  batch %9.3f [%9.3f .. %9.3f] ms %9.0f files/s spread %4.1f %%   loop %9.3f [%9.3f .. %9.3f] ms %9.0f files/s spread %4.1f %%   loop / batch %.2f%s%s" % (
                    n, w, h, preset, kind, mb, min(tb), max(tb), n / mb * 1e3, (max(tb) - min(tb)) / mb * 100,
                    ml, min(tl), max(tl), n / ml * 1e3, (max(tl) - min(tl)) / ml * 100, ml / mb,
                    "" if mb < ml else "   THE BATCH DOES NOT WIN HERE", "" if same else "   FILES DIFFER")
                print(row, flush=True)
                lines.append(row)
                for ln in traced(batch):
                    lines.append("      " + ln)
                with open(path, "w") as f:  # (kept current: a later shape may run out of time)
                    f.write("\n".join(lines) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
