#!/usr/bin/env python3
"""Timing of the PNG lossy mode (pixo_hip_png_quantize_device) on 512x512, 2048x2048 and 4096x4096 RGBA images of 1,000
colours, about 30 % of them not opaque (Auto fires, dithering on: the options of the wasm's `lossy` argument).

Per size: the whole call (device events around >= 10 calls after warm-up), then the stages of one call as the library's
`trace` switch reports them: per stage the time between two device events on the library's stream (what the device spent)
and the host's wall time over the same stage (launches, copies and the host's own work included; for the host part this is
the figure that counts): gather (kernel + the copy of the samples), host part (sort, run lengths, gate, median cut),
k-means (two rounds: upload, kernel, sums down, centroids), LUT, dither.  The map kernel is timed by a second call with
dithering off.  Beside them: the reference's own wasm build on the same pixels (`--wasm`: run where node and
oracle/_ref/pixo_bg.wasm are, i.e. on a CPU; its figures are then pasted into WASM_MS below), the LUT kernel's arithmetic
bound, and the dither's steps.

    python tools/png_quantize_timing.py [--reps 10] > profiles/png_quantize_timing.txt
    python tools/png_quantize_timing.py --wasm        (CPU only: prints the reference's ms per size)
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (512, 2048, 4096)
# encodePng(..., preset 0, lossy) of the reference's wasm build under node on the build machine's CPU, ms (best of 3), same pixels
WASM_MS = {512: 1060, 2048: 6125, 4096: 20372}


def pixels(n):
    import png_quantize_cases as QC
    return QC.make_input(dict(gen="pal", w=n, h=n, color_type=3, preset=0, seed=7, n=1000))


def wasm():
    with tempfile.TemporaryDirectory() as tmp:
        cases = []
        for n in SIZES:
            inp = os.path.join(tmp, "in%d.bin" % n)
            pixels(n).tofile(inp)
            cases.append(dict(kind="png", input=inp, w=n, h=n, color_type=3, preset=0, lossy=True, repeat=3))
        mp = os.path.join(tmp, "m.json")
        json.dump({"cases": cases}, open(mp, "w"))
        out = subprocess.run(["node", "--max-old-space-size=4096", os.path.join(ROOT, "oracle", "ref_wasm.js"), mp], stdout=subprocess.PIPE,
                             check=True).stdout.decode().strip().splitlines()
    for n, line in zip(SIZES, out):
        r = json.loads(line)
        print(n, "%.0f ms (best of %d), %d bytes" % (min(r["ms"]), len(r["ms"]), r["len"]) if r["ok"] else r)


def traced(fn):
    """fn() with the `trace` switch on; -> {stage: (host ms, device-event ms)} from what the library wrote to stderr"""
    from pixo_amd import _lib
    L = _lib.load()
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            L.pixo_hip_debug_configure(b"trace")
            fn()
        finally:
            L.pixo_hip_debug_configure(None)
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode()
    return {m.group(1).strip(): (float(m.group(2)), float(m.group(3)))
            for m in re.finditer(r"\[pixo_hip\] png quantize: (.+?)\s+([0-9.]+) ms\s+device events\s+([0-9.]+) ms", text)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--wasm", action="store_true")
    a = ap.parse_args()
    if a.wasm:
        return wasm()
    import torch
    from pixo_amd import png
    assert torch.cuda.is_available(), "needs the GPU: no timing is taken on a CPU"
    print("# PNG lossy mode, RGBA, 1,000 colours (about 30 %% not opaque), Auto / 256 colours; %s; %d timed calls after 2 warm-up calls" % (
        torch.cuda.get_device_name(0), a.reps))
    print("# whole call: device events, median [min .. max] ms; stages (switch `trace`, one call): device events on the library's stream | host wall time")
    for n in SIZES:
        px = pixels(n)
        d_px = torch.from_numpy(px.copy()).cuda()
        d_idx = torch.empty(n * n, dtype=torch.uint8, device="cuda")
        o = png.PngOptions.from_preset_with_lossless(n, n, 0, False)
        plain = png.PngOptions.from_preset_with_lossless(n, n, 0, False)
        plain.quantization.dithering = False

        def call(opts=o):
            q = png.quantize_device(d_px, opts, d_idx)
            assert q.applied and len(q.palette) == 256
        ms = {}
        for name, opts in (("dithering", o), ("no dithering", plain)):
            for _ in range(2):
                call(opts)
            t = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(opts)
                e1.record()
                torch.cuda.synchronize()
                t.append(e0.elapsed_time(e1))
            ms[name] = (float(np.median(t)), min(t), max(t))
        st, st_plain = traced(call), traced(lambda: call(plain))
        bands = (n + 63) // 64
        print("\n## %dx%d (%d pixels, %d bands of 64 rows)" % (n, n, n * n, bands))
        for name in ms:
            print("quantize_device, %-13s %9.3f [%.3f .. %.3f] ms" % ((name + ":",) + ms[name]))
        nan = (float("nan"), float("nan"))
        for k in ("gather", "host part", "k-means", "LUT", "dither"):
            print("  stage %-10s device %9.3f ms | host %9.3f ms" % (k, st.get(k, nan)[1], st.get(k, nan)[0]))
        print("  stage %-10s device %9.3f ms | host %9.3f ms   (the call without dithering)" % ("map", st_plain.get("map", nan)[1], st_plain.get("map", nan)[0]))
        assert "dither gave up" not in st, "the chained dither gave up and ran band by band"
        total = sum(v[0] for v in st.values())
        print("  host part's share of the staged call (host wall times): %.1f %%" % (100 * st.get("host part", nan)[0] / total if total else float("nan")))
        # The compiled inner loop, per palette entry and thread (four cells): about 30 full-rate VALU instructions and 4 v_mad_u64_u32
        # at a quarter of that rate; 65,536 threads x 256 entries; full rate = 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6 T lanes/s
        full, quarter = 65536 * 256 * 30, 65536 * 256 * 4
        print("  LUT: %.2f G full-rate + %.2f G quarter-rate lane-instructions = %.1f us at 78.6 T/s (256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz)" % (
            full / 1e9, quarter / 1e9, (full + 4 * quarter) / 78.6e12 * 1e6))
        print("  dither: %d steps per band (W + 126), %d dependent steps in all (W + 2H), %.3f us per dependent step (device events)" % (
            n + 126, n + 2 * n, 1000 * st.get("dither", nan)[1] / (3 * n)))
        w = WASM_MS.get(n)
        print("  reference wasm (node, CPU, preset 0, whole encodePng): %s" % ("%.0f ms" % w if w else "not recorded"))


if __name__ == "__main__":
    main()
