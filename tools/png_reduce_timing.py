#!/usr/bin/env python3
"""Timing of the PNG prepare path on 4096x4096 RGBA, four contents: noise with alpha >= 1 (nothing applies), opaque
photo-like (-> RGB), 16 colours (-> 4-bit palette), 256 grays (-> 8-bit palette).  Device events around >= 20 calls after
warm-up.  Per content: prepare_device, pixo_hip_png_filter_device on the same pixels in the same run (a: the price of
asking), the host model's time for the same image (b), bytes the passes read and write, and the same-run streaming
kernel of comparable shape (pixo_hip_debug_stream_io: a copy of the pixels, read + written once).

    python tools/png_reduce_timing.py [--size 4096] [--reps 20] [--once] > profiles/png_reduce_timing.txt

--once: one warm call per content and nothing else (for a kernel trace: rocprofv3 --kernel-trace --stats -- python ... --once)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def contents(n):
    rng = np.random.RandomState(7)
    y, x = np.mgrid[0:n, 0:n]
    noise = rng.randint(0, 256, (n, n, 4)).astype(np.uint8)
    noise[:, :, 3] |= 1
    photo = np.stack([(x * 255 // n + rng.randint(0, 8, (n, n))) & 255, (y * 255 // n + rng.randint(0, 8, (n, n))) & 255,
                      ((x + y) * 255 // (2 * n) + rng.randint(0, 8, (n, n))) & 255, np.full((n, n), 255)], axis=2).astype(np.uint8)
    cols = rng.randint(0, 256, (16, 4)).astype(np.uint8)
    cols[:, 3] = 255
    idx = ((x // 61 + y // 47) % 16)
    speck = rng.rand(n, n) < 0.05
    idx[speck] = rng.randint(0, 16, int(speck.sum()))
    g = ((x + y) * 255 // (2 * n) + rng.randint(0, 3, (n, n))).clip(0, 255).astype(np.uint8)
    grays = np.stack([g, g, g, np.full_like(g, 255)], axis=2)
    return [("noise alpha>=1 (nothing applies)", noise), ("opaque photo-like (-> RGB)", photo), ("16 colours (-> 4-bit palette)", cols[idx]),
            ("256 grays (-> 8-bit palette)", grays)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    import png_reduce_model as M
    from pixo_amd import jpeg, png
    assert torch.cuda.is_available(), "needs the GPU: no timing is taken on a CPU"
    n = a.size
    o = png.PngOptions.builder(n, n).preset(1).build()
    print("# PNG prepare path, %dx%d RGBA, preset 1 (Adaptive, all reductions); %s; %d timed calls after 3 warm-up calls" % (
        n, n, torch.cuda.get_device_name(0), a.reps))
    print("# times: device events around the whole synchronous call (host decisions and their copies included), median [min .. max] ms")

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return "%.3f [%.3f .. %.3f]" % (ts[len(ts) // 2], ts[0], ts[-1])

    d_out = torch.empty(o.full_size(), dtype=torch.uint8, device="cuda:0")
    d_copy = torch.empty(n * n * 4, dtype=torch.uint8, device="cuda:0")
    for name, img in contents(n):
        px = np.ascontiguousarray(img).reshape(-1)
        d_px = torch.from_numpy(px).to("cuda:0")
        torch.cuda.synchronize()
        length, lay, adler = png.prepare_device(d_px, o, d_out)
        if a.once:
            print(name, length, lay)
            continue
        t0 = time.perf_counter()
        want, wlay, wad = M.prepare(px, n, n, 3, M.Opts.preset(1))
        t_model = time.perf_counter() - t0
        assert M.layout_of(lay) == wlay and adler == wad and np.array_equal(d_out.cpu().numpy()[:length], want), name
        src = n * n * 4
        pal = lay.color_type_byte == 3
        rows = lay.row_bytes * n
        moved = dict(analyse=(src, 0), index=(src, n * n) if pal else None, cooccurrence=(n * n * 3, 0) if pal else None,
                     convert=((n * n if pal else src), rows) if rows != src else None, filter=(rows, rows + n))
        print("\n## %s -> %r, stream %d bytes (checked against the host model)" % (name, lay, length))
        print("bytes read + written per pass (analyse: at most; it leaves early when every question is answered): " +
              ", ".join("%s %d + %d" % (k, v[0], v[1]) for k, v in moved.items() if v))
        print("prepare_device                         %s ms" % timed(lambda: png.prepare_device(d_px, o, d_out)))
        print("png_filter_device, same pixels (RGBA)  %s ms" % timed(lambda: png.apply_filters_device(d_px, n, n, 4, d_out, png.FilterStrategy.ADAPTIVE)))
        wg = src // 16 // 192
        print("stream_io copy of the pixels, 1 x 16 B %s ms" % timed(lambda: jpeg.debug_stream_io(d_px, d_copy, wg, 1, 1)))
        print("stream_io copy of the pixels, 4 x 16 B %s ms" % timed(lambda: jpeg.debug_stream_io(d_px, d_copy, wg // 4, 4, 4)))
        print("host model (numpy + C oracle filters)  %.0f ms" % (t_model * 1e3))


if __name__ == "__main__":
    main()
