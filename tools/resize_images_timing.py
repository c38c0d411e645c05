#!/usr/bin/env python3
"""Time of the resize images entry (pixo_hip_resize_images_device: sources and destinations of individual sizes and colour
types, one flat launch per pass and pixel size) against a loop of pixo_hip_resize_device calls over the same images in the same
run — and, where all images are equal, against pixo_hip_resize_batch_device too.

Workloads, each for nearest, bilinear and Lanczos3:
  (a) 64 sources of 1280-1920 x 720-1080, Rgb and Rgba mixed, fitted into 320x320
  (b) 1024 sources of 64-256 a side in all four colour types, fitted into 48x48
  (c) 64 equal 1920x1080 Rgb sources to 320x180
The destination sizes are pixo_hip_resize_images_fit's.  Every timed pass uses the next of a ring of source and destination
blocks whose total exceeds the 256 MiB Infinity Cache, so the bytes come from HBM.  Two figures per form: DEVICE, HIP events
around a block of passes enqueued on one stream (us per pass, median and minimum of 5 blocks, the forms alternating; it holds
whatever host time the device had to wait for); WALL, the host clock around one pass ending in a synchronise, the host's
table building included (median of 5, the forms alternating).  All forms are called through ctypes with their arguments
prepared beforehand, after a warm-up of every block through every form.  Before timing, the images entry's bytes are compared
with the loop's.

    python tools/resize_images_timing.py [--out profiles/resize_images_timing.txt]
"""
import argparse
import ctypes as C
import os
import random
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import profile_meta  # noqa: E402
import resize_cases as RC  # noqa: E402
import synth  # noqa: E402
from pixo_amd import _lib  # noqa: E402

RING_BYTES = 320 << 20
BLOCKS = 5


def workloads():
    rng = random.Random(355)
    a = [(rng.randint(1280, 1920), rng.randint(720, 1080), rng.choice([2, 3])) for _ in range(64)]
    b = [(rng.randint(64, 256), rng.randint(64, 256), i % 4) for i in range(1024)]
    c = [(1920, 1080, 2)] * 64
    return [("a: 64 x 1280-1920 x 720-1080, Rgb/Rgba -> fit 320x320", a, (320, 320)),
            ("b: 1024 x 64-256 a side, 4 colour types -> fit 48x48", b, (48, 48)),
            ("c: 64 x 1920x1080 Rgb -> 320x180", c, (320, 180))]


def timed(forms, ring, per):
    """(device us per pass: median, min), (wall us per pass: median) of each form"""
    dev = [[] for _ in forms]
    wall = [[] for _ in forms]
    for b in range(BLOCKS):
        for k, fn in enumerate(forms):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(per):
                fn((b * per + i) % ring)
            e1.record()
            torch.cuda.synchronize()
            dev[k].append(e0.elapsed_time(e1) / per * 1e3)
    for b in range(BLOCKS):
        for k, fn in enumerate(forms):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(b % ring)
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e6)
    return [(statistics.median(d), min(d), statistics.median(w)) for d, w in zip(dev, wall)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_images_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resize_images_timing.py measures on the GPU; there is no CPU fallback"
    L = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    s_arg = C.c_void_p(stream) if stream else None
    meta = profile_meta.meta("resize_images")
    lines = ["resize images against a loop of single calls, %s on %s (%s)" % (meta["library_version"], torch.cuda.get_device_name(0), socket.gethostname()),
             "kernel sources %s: %s" % (meta["kernel_source_hash"], " ".join(meta["kernel_sources"])),
             "a pass = all images of a workload; ring of blocks > %d MiB; us per pass; device = HIP events around a block of passes on one stream, median (min) of %d"
             % (RING_BYTES >> 20, BLOCKS),
             "alternating blocks; wall = host clock around one pass and its synchronise, median of %d; loop = pixo_hip_resize_device per image; batch = pixo_hip_resize_batch_device" % BLOCKS,
             "%-9s %21s %10s %21s %10s %11s %11s %21s %10s %12s" % ("algorithm", "images device", "wall", "loop device", "wall", "loop/images", "wall ratio",
                                                                   "batch device", "wall", "images/batch")]
    for title, shapes, box in workloads():
        n = len(shapes)
        src, at = (_lib.PngImageC * n)(), 0
        for i, (w, h, ct) in enumerate(shapes):
            src[i].offset, src[i].width, src[i].height, src[i].color_type = at, w, h, ct
            at = (at + w * h * (ct + 1) + 15) // 16 * 16
        src_end = at
        dst, total = (_lib.PngImageC * n)(), C.c_size_t()
        assert L.pixo_hip_resize_images_fit(src, n, box[0], box[1], 0, dst, C.byref(total)) == 0, L.pixo_hip_last_error()
        dst_end = total.value
        equal = len(set(shapes)) == 1
        ring = RING_BYTES // (src_end + dst_end) + 2
        seed_px = torch.from_numpy(synth.lcg_bytes(min(src_end, 16 << 20), 5)).to("cuda:0")  # (content generation is host time: 16 MiB, repeated)
        px = seed_px.repeat(-(-src_end // seed_px.numel()))[:src_end].contiguous()
        sets = [px.clone() for _ in range(ring)]
        d_images = [torch.zeros(dst_end, dtype=torch.uint8, device="cuda:0") for _ in range(ring)]
        d_loop = [torch.zeros(dst_end, dtype=torch.uint8, device="cuda:0") for _ in range(ring)]
        d_batch = [torch.zeros(dst_end, dtype=torch.uint8, device="cuda:0") for _ in range(ring)] if equal else []
        lines.append("%s   (%d source bytes, %d destination bytes, ring %d)" % (title, src_end, dst_end, ring))
        print(lines[-1], flush=True)
        for algo in (0, 1, 2):
            opts = [_lib.ResizeOptionsC(src[i].width, src[i].height, dst[i].width, dst[i].height, src[i].color_type, algo) for i in range(n)]
            sources = []
            for s in sets:
                arr = (_lib.ResizeSourceC * n)()
                for i in range(n):
                    arr[i] = _lib.ResizeSourceC(s.data_ptr() + src[i].offset, src[i].width, src[i].height)
                sources.append(arr)

            def images(k):
                rc = L.pixo_hip_resize_images_device(sets[k].data_ptr(), src, d_images[k].data_ptr(), dst, n, algo, s_arg)
                assert rc == 0, L.pixo_hip_last_error()

            def loop(k):
                base, out = sets[k].data_ptr(), d_loop[k].data_ptr()
                for i in range(n):
                    rc = L.pixo_hip_resize_device(base + src[i].offset, C.byref(opts[i]), out + dst[i].offset, s_arg)
                    assert rc == 0, L.pixo_hip_last_error()

            def batch(k):  # (equal images: the fitted layout is then back to back only when an image's bytes are a multiple of 16)
                rc = L.pixo_hip_resize_batch_device(sources[k], n, dst[0].width, dst[0].height, shapes[0][2], algo, d_batch[k].data_ptr(), s_arg)
                assert rc == 0, L.pixo_hip_last_error()

            forms = [images, loop] + ([batch] if equal else [])
            for k in range(ring):  # warm-up: every block through every form
                for fn in forms:
                    fn(k)
            torch.cuda.synchronize()
            same = all(torch.equal(d_images[k], d_loop[k]) for k in range(ring))
            got = timed(forms, ring, max(ring, 3))
            (i_us, i_min, i_wall), (l_us, l_min, l_wall) = got[0], got[1]
            row = "%-9s %10.1f (%8.1f) %10.1f %10.1f (%8.1f) %10.1f %11.2f %11.2f" % (RC.ALGO_NAMES[algo], i_us, i_min, i_wall, l_us, l_min, l_wall, l_us / i_us, l_wall / i_wall)
            if equal:
                b_us, b_min, b_wall = got[2]
                row += " %10.1f (%8.1f) %10.1f %12.3f" % (b_us, b_min, b_wall, i_us / b_us)
                row += "" if i_us <= b_us * 1.03 else "   SLOWER THAN THE BATCH ENTRY"
            row += ("" if i_us <= l_us * 1.03 and i_wall <= l_wall * 1.03 else "   THE IMAGES ENTRY IS SLOWER THAN THE LOOP HERE") + ("" if same else "   OUTPUTS DIFFER")
            lines.append(row)
            print(row, flush=True)
            with open(a.out, "w") as f:  # (kept current: a later row may run out of time)
                f.write("\n".join(lines) + "\n")
        del sets, d_images, d_loop, d_batch, px
    print("wrote", a.out)


if __name__ == "__main__":
    main()
