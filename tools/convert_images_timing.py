#!/usr/bin/env python3
"""Time of the colour-conversion entries (pixo_hip_convert_images_device: N images of individual sizes and colour types, one
launch per conversion and alignment class present) on one GPU, in one run:

  (a) every kind over 64 images of 1920x1080, aligned form, against pixo_hip_debug_stream_copy moving the same traffic — a
      copy of (bytes in + bytes out) / 2 bytes reads and writes that many bytes in all — timed in the same run;
  (b) the images entry against a loop of pixo_hip_convert_device calls over the same images, target OPAQUE, on
        a: 64 images of 1280-1920 x 720-1080 in all four colour types
        b: 1024 thumbnails of 64-256 a side in all four colour types
        c: 64 equal 1920x1080 Rgba images — there also against ONE single call on an image of 64 x the pixels;
  (c) workload c with the source block one byte behind a multiple of 16 (every image takes the byte form) against the aligned form.

Every timed pass uses the next of a ring of source and destination blocks whose total exceeds the 256 MiB Infinity Cache, so
the bytes come from HBM.  DEVICE: HIP events around a block of passes enqueued on one stream (us per pass, median and minimum
of 5 blocks, the forms alternating).  WALL: the host clock around one pass ending in a synchronise, the host's table building
included (median of 5).  All forms are called through ctypes with their arguments prepared beforehand, after a warm-up of
every block through every form.  Before timing, the images entry's bytes are compared with the loop's.

    python tools/convert_images_timing.py [--out profiles/convert_images_timing.txt]
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
import synth  # noqa: E402
from pixo_amd import _lib  # noqa: E402

RING_BYTES = 320 << 20
BLOCKS = 5
COPY_CHUNK = 24576
KINDS = [("copy Rgb", 2, 2), ("GrayAlpha -> Gray", 1, 0), ("Rgba -> Rgb", 3, 2), ("Rgb -> Gray", 2, 0), ("Rgba -> Gray", 3, 0)]


def timed(forms, ring, per):
    """(device us per pass: median, min, wall us per pass: median) of each form"""
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


class Job:
    """The records of `shapes` (w, h, source colour type) -> `dst_cts`, a ring of blocks, and the forms that run them"""

    def __init__(self, L, s_arg, shapes, dst_cts, src_shift=0):
        self.L, self.s_arg, self.n = L, s_arg, len(shapes)
        n = self.n
        self.src, at = (_lib.PngImageC * n)(), 0
        for i, (w, h, ct) in enumerate(shapes):
            self.src[i].offset, self.src[i].width, self.src[i].height, self.src[i].color_type = at, w, h, ct
            at = (at + w * h * (ct + 1) + 15) // 16 * 16
        self.src_end = at
        self.dst, at = (_lib.PngImageC * n)(), 0
        for i, ((w, h, _), ct) in enumerate(zip(shapes, dst_cts)):
            self.dst[i].offset, self.dst[i].width, self.dst[i].height, self.dst[i].color_type = at, w, h, ct
            at = (at + w * h * (ct + 1) + 15) // 16 * 16
        self.dst_end = at
        self.ring = RING_BYTES // (self.src_end + self.dst_end) + 2
        seed_px = torch.from_numpy(synth.lcg_bytes(min(self.src_end, 16 << 20), 5)).to("cuda:0")  # (content generation is host time: 16 MiB, repeated)
        px = seed_px.repeat(-(-self.src_end // seed_px.numel()))[:self.src_end].contiguous()
        self.shift = src_shift
        self.sets = []
        for _ in range(self.ring):
            t = torch.empty(self.src_end + 16, dtype=torch.uint8, device="cuda:0")
            t[src_shift:src_shift + self.src_end] = px
            self.sets.append(t)
        self.d_images = [torch.zeros(self.dst_end, dtype=torch.uint8, device="cuda:0") for _ in range(self.ring)]
        self.d_loop = [torch.zeros(self.dst_end, dtype=torch.uint8, device="cuda:0") for _ in range(self.ring)]
        self.copy_bytes = (self.src_end + self.dst_end) // 2 // COPY_CHUNK * COPY_CHUNK

    def images(self, k):
        rc = self.L.pixo_hip_convert_images_device(self.sets[k].data_ptr() + self.shift, self.src, self.d_images[k].data_ptr(), self.dst, self.n, self.s_arg)
        assert rc == 0, self.L.pixo_hip_last_error()

    def loop(self, k):
        base, out, src, dst, L, s_arg = self.sets[k].data_ptr() + self.shift, self.d_loop[k].data_ptr(), self.src, self.dst, self.L, self.s_arg
        for i in range(self.n):
            rc = L.pixo_hip_convert_device(base + src[i].offset, src[i].width, src[i].height, src[i].color_type, dst[i].color_type, out + dst[i].offset, s_arg)
            assert rc == 0, L.pixo_hip_last_error()

    def copy(self, k):  # (the source block holds at least (in + out) / 2 bytes only when in >= out: true of every kind)
        rc = self.L.pixo_hip_debug_stream_copy(self.sets[k].data_ptr(), self.d_loop[k].data_ptr() if self.copy_bytes <= self.dst_end else self.big[k].data_ptr(),
                                               self.copy_bytes, self.s_arg)
        assert rc == 0, self.L.pixo_hip_last_error()

    def run(self, forms):
        if self.copy in forms and self.copy_bytes > self.dst_end:
            self.big = [torch.zeros(self.copy_bytes, dtype=torch.uint8, device="cuda:0") for _ in range(self.ring)]
        for k in range(self.ring):  # warm-up: every block through every form
            for fn in forms:
                fn(k)
        torch.cuda.synchronize()
        return timed(forms, self.ring, max(self.ring, 3))

    def same(self):
        return all(torch.equal(a, b) for a, b in zip(self.d_images, self.d_loop))


def opaque(ct):
    return {0: 0, 1: 0, 2: 2, 3: 2}[ct]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_images_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "convert_images_timing.py measures on the GPU; there is no CPU fallback"
    L = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    s_arg = C.c_void_p(stream) if stream else None
    meta = profile_meta.meta("convert_images")
    lines = ["colour conversion of images, %s on %s (%s)" % (meta["library_version"], torch.cuda.get_device_name(0), socket.gethostname()),
             "kernel sources %s: %s" % (meta["kernel_source_hash"], " ".join(meta["kernel_sources"])),
             "a pass = all images of a workload; ring of blocks > %d MiB; us per pass; device = HIP events around a block of passes on one stream, median (min) of %d"
             % (RING_BYTES >> 20, BLOCKS),
             "alternating blocks; wall = host clock around one pass and its synchronise, median of %d" % BLOCKS]

    def emit(row):
        lines.append(row)
        print(row, flush=True)
        with open(a.out, "w") as f:  # (kept current: a later row may run out of time)
            f.write("\n".join(lines) + "\n")

    emit("(a) 64 x 1920x1080 per kind, aligned form, against a plain copy of the same traffic (pixo_hip_debug_stream_copy of (in + out) / 2 bytes)")
    emit("%-18s %12s %12s %21s %10s %21s %12s %12s" % ("kind", "bytes in", "bytes out", "images device", "GB/s", "copy device", "GB/s", "images/copy"))
    for name, s_ct, d_ct in KINDS:
        job = Job(L, s_arg, [(1920, 1080, s_ct)] * 64, [d_ct] * 64)
        (i_us, i_min, _), (c_us, c_min, _) = job.run([job.images, job.copy])
        traffic = job.src_end + job.dst_end
        emit("%-18s %12d %12d %10.1f (%8.1f) %10.0f %10.1f (%8.1f) %12.0f %12.2f" % (name, job.src_end, job.dst_end, i_us, i_min, traffic / i_us / 1e3, c_us, c_min,
                                                                                      2 * job.copy_bytes / c_us / 1e3, i_us / c_us))
        del job
    rng = random.Random(355)
    wa = [(rng.randint(1280, 1920), rng.randint(720, 1080), i % 4) for i in range(64)]
    wb = [(rng.randint(64, 256), rng.randint(64, 256), i % 4) for i in range(1024)]
    wc = [(1920, 1080, 3)] * 64
    emit("(b) the images entry against a loop of pixo_hip_convert_device calls, target OPAQUE")
    emit("%-58s %21s %10s %21s %10s %11s %11s" % ("workload", "images device", "wall", "loop device", "wall", "loop/images", "wall ratio"))
    for title, shapes in (("a: 64 x 1280-1920 x 720-1080, 4 colour types", wa), ("b: 1024 x 64-256 a side, 4 colour types", wb), ("c: 64 x 1920x1080 Rgba", wc)):
        job = Job(L, s_arg, shapes, [opaque(ct) for _, _, ct in shapes])
        (i_us, i_min, i_wall), (l_us, l_min, l_wall) = job.run([job.images, job.loop])
        emit("%-58s %10.1f (%8.1f) %10.1f %10.1f (%8.1f) %10.1f %11.2f %11.2f%s%s" % (
            title, i_us, i_min, i_wall, l_us, l_min, l_wall, l_us / i_us, l_wall / i_wall,
            "" if i_us <= l_us * 1.03 and i_wall <= l_wall * 1.03 else "   THE IMAGES ENTRY IS SLOWER THAN THE LOOP HERE", "" if job.same() else "   OUTPUTS DIFFER"))
        if shapes is wc:
            c_images = (i_us, i_min)
        del job
    one = Job(L, s_arg, [(1920, 1080 * 64, 3)], [2])
    (o_us, o_min, o_wall), (r_us, r_min, _) = one.run([one.loop, one.images])
    emit("c as ONE image of 1920 x 69120: single entry %.1f (%.1f) us device, %.1f wall; the images entry on that one record %.1f (%.1f); the 64-image entry / single = %.3f"
         % (o_us, o_min, o_wall, r_us, r_min, c_images[0] / o_us))
    del one
    emit("(c) workload c with the source block one byte behind a multiple of 16: the byte form against the aligned form")
    odd = Job(L, s_arg, wc, [2] * 64, src_shift=1)
    (b_us, b_min, b_wall), = odd.run([odd.images])
    emit("byte form %.1f (%.1f) us device, %.1f wall; aligned form %.1f (%.1f): byte / aligned = %.2f" % (b_us, b_min, b_wall, c_images[0], c_images[1], b_us / c_images[0]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
