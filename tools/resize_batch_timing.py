#!/usr/bin/env python3
"""Device time of a resize batch (pixo_hip_resize_batch_device: one launch per pass for all images) against a loop of
pixo_hip_resize_device calls over the same sources in the same run, and both against a plain copy of the bytes they move.

Workloads: 64 x 1920x1080 RGB -> 320x180 and 64 x 256x256 RGB -> 64x64; nearest, bilinear, Lanczos3; sources all of the nominal
size ("equal") and of individual sizes down to three quarters of it ("ragged").  Every timed pass uses the next of a ring of
source sets and destination blocks whose total exceeds the 256 MiB Infinity Cache, so the bytes come from HBM.  HIP events
around blocks of passes on one stream, batch and loop blocks alternating; median and minimum of 7 blocks after a warm-up of
every set through both.  Both forms are called through ctypes with their arguments prepared beforehand.  The copy is
pixo_hip_debug_stream_copy over the set's source + destination bytes (Lanczos3: plus twice the intermediate), rounded up to
its 24 KiB granule.  Before timing, the batch's block is compared with the loop's.

    python tools/resize_batch_timing.py [--out profiles/resize_batch_timing.txt]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import profile_meta  # noqa: E402
import resize_cases as RC  # noqa: E402
import synth  # noqa: E402
from pixo_amd import _lib  # noqa: E402

WORKLOADS = [(64, 1920, 1080, 320, 180), (64, 256, 256, 64, 64)]
CT, BPP = 2, 3
RING_BYTES = 320 << 20
GRANULE = 24576
BLOCKS = 7


def sizes_of(kind, n, w, h):
    if kind == "equal":
        return [(w, h)] * n
    return [(w - (i * 37) % (w // 4), h - (i * 53) % (h // 4)) for i in range(n)]


def mid_stride(dw):
    return (dw * BPP + 15) // 16 * 16


def blocks_of(forms, ring, per):
    """us per pass of each form: BLOCKS blocks of `per` passes each, the forms alternating"""
    us = [[] for _ in forms]
    for b in range(BLOCKS):
        for k, fn in enumerate(forms):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(per):
                fn((b * per + i) % ring)
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) / per * 1e3)
    return [(statistics.median(u), min(u)) for u in us]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_batch_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resize_batch_timing.py measures on the GPU; there is no CPU fallback"
    L = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    s_arg = C.c_void_p(stream) if stream else None
    meta = profile_meta.meta("resize_batch")
    lines = ["resize batch against a loop of single calls, %s on %s (%s)" % (meta["library_version"], torch.cuda.get_device_name(0), socket.gethostname()),
             "kernel sources %s: %s" % (meta["kernel_source_hash"], " ".join(meta["kernel_sources"])),
             "Rgb; a pass = all images of a set; ring of sets > %d MiB; us per pass, median (min) of %d alternating blocks, HIP events on one stream;"
             % (RING_BYTES >> 20, BLOCKS),
             "copy = pixo_hip_debug_stream_copy of the set's src + dst bytes (lanczos3: + 2 x intermediate)",
             "%-26s %-7s %-9s %19s %19s %12s %17s %8s %8s" % ("workload", "sources", "algorithm", "batch us", "loop us", "loop / batch", "copy us", "batch/cp", "loop/cp")]
    for n, w, h, dw, dh in WORKLOADS:
        each = dw * dh * BPP
        for kind in ("equal", "ragged"):
            sizes = sizes_of(kind, n, w, h)
            at = [0]
            for sw, sh in sizes:
                at.append(at[-1] + (sw * sh * BPP + 15) // 16 * 16)
            src_bytes = sum(sw * sh * BPP for sw, sh in sizes)
            mid_bytes = sum(mid_stride(dw) * sh for _, sh in sizes)
            ring = RING_BYTES // (at[-1] + n * each) + 2
            seed_px = torch.from_numpy(synth.lcg_bytes(min(at[-1], 16 << 20), 5)).to("cuda:0")  # (content generation is host time: 16 MiB, repeated)
            px = seed_px.repeat(-(-at[-1] // seed_px.numel()))[:at[-1]].contiguous()
            sets = [px.clone() for _ in range(ring)]
            d_batch = [torch.zeros(n * each, dtype=torch.uint8, device="cuda:0") for _ in range(ring)]
            d_loop = [torch.zeros(n * each, dtype=torch.uint8, device="cuda:0") for _ in range(ring)]
            arrays = []
            for s in sets:
                arr = (_lib.ResizeSourceC * n)()
                for i, (sw, sh) in enumerate(sizes):
                    arr[i] = _lib.ResizeSourceC(s.data_ptr() + at[i], sw, sh)
                arrays.append(arr)
            for algo in (0, 1, 2):
                opts = [_lib.ResizeOptionsC(sw, sh, dw, dh, CT, algo) for sw, sh in sizes]
                moved = src_bytes + n * each + (2 * mid_bytes if algo == 2 else 0)
                copy_bytes = (moved + GRANULE - 1) // GRANULE * GRANULE
                c_ring = RING_BYTES // (2 * copy_bytes) + 2
                c_src = [torch.zeros(copy_bytes, dtype=torch.uint8, device="cuda:0") for _ in range(c_ring)]
                c_dst = [torch.zeros(copy_bytes, dtype=torch.uint8, device="cuda:0") for _ in range(c_ring)]

                def batch(k):
                    rc = L.pixo_hip_resize_batch_device(arrays[k], n, dw, dh, CT, algo, d_batch[k].data_ptr(), s_arg)
                    assert rc == 0, L.pixo_hip_last_error()

                def loop(k):
                    base, dst = sets[k].data_ptr(), d_loop[k].data_ptr()
                    for i in range(n):
                        rc = L.pixo_hip_resize_device(base + at[i], C.byref(opts[i]), dst + i * each, s_arg)
                        assert rc == 0, L.pixo_hip_last_error()

                def copy(k):
                    rc = L.pixo_hip_debug_stream_copy(c_src[k % c_ring].data_ptr(), c_dst[k % c_ring].data_ptr(), copy_bytes, s_arg)
                    assert rc == 0, L.pixo_hip_last_error()

                for k in range(ring):  # warm-up: every set through both forms
                    batch(k)
                    loop(k)
                    copy(k)
                torch.cuda.synchronize()
                same = all(torch.equal(d_batch[k], d_loop[k]) for k in range(ring))
                per = max(ring, 4)
                (b_us, b_min), (l_us, l_min) = blocks_of([batch, loop], ring, per)
                (c_us, c_min), = blocks_of([copy], ring, max(per, 8))
                lines.append("%-26s %-7s %-9s %9.1f (%7.1f) %9.1f (%7.1f) %12.2f %8.1f (%6.1f) %8.2f %8.2f%s%s" % (
                    "%d x %dx%d->%dx%d" % (n, w, h, dw, dh), kind, RC.ALGO_NAMES[algo], b_us, b_min, l_us, l_min, l_us / b_us, c_us, c_min,
                    b_us / c_us, l_us / c_us, "" if b_us <= l_us * 1.03 else "   THE BATCH IS SLOWER HERE", "" if same else "   OUTPUTS DIFFER"))
                print(lines[-1], flush=True)
                del c_src, c_dst
                with open(a.out, "w") as f:  # (kept current: a later row may run out of time)
                    f.write("\n".join(lines) + "\n")
            del sets, d_batch, d_loop, px
    print("wrote", a.out)


if __name__ == "__main__":
    main()
