#!/usr/bin/env python3
"""A JPEG decode batch (pixo_hip_jpeg_decode_batch_device: the entropy decodes on a pool of host threads, the records and the
coefficients up in two copies, one launch per class) on the same build in the same run against
  * a loop of pixo_hip_jpeg_decode_device calls over the same files;
  * what callers do today: Pillow (libjpeg-turbo) on the same number of host threads, the pixels joined and uploaded in one copy;
and the kernel's device time against a plain device copy that moves as many bytes as the kernel reads and writes.

Workloads: 64 files of 1920x1080 at quality 80, 4:2:0 and 4:4:4 (8 distinct scenes, each eight times in the list), and 1024
files of 64..256 pixels a side in all four classes.  Wall time of a call up to the synchronisation of its stream, median and
minimum of ROUNDS rounds after WARMUP warm-up rounds, the forms alternating; the legs — entropy decode (host clock), uploads,
kernels, copy down (HIP events) — from pixo_hip_debug_jpeg_decode_batch_timed, median of the same rounds.  Before timing, the
batch's images are compared with Pillow's.

    python tools/jpeg_decode_batch_timing.py [--out profiles/jpeg_decode_batch_timing.txt]
"""
import argparse
import io
import os
import socket
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image, features  # noqa: E402

import synth  # noqa: E402
from pixo_amd import _lib, decode  # noqa: E402

WARMUP, ROUNDS, THREADS = 2, 5, 8


def write(px, w, h, mode, quality=80):
    im = Image.fromarray(px.reshape(h, w, 3))
    b = io.BytesIO()
    if mode == "gray":
        im.convert("L").save(b, "JPEG", quality=quality)
    else:
        im.save(b, "JPEG", quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[mode])
    return b.getvalue()


def workloads():
    scenes = [synth.scene(1920, 1080, 300 + k) for k in range(8)]
    out = {}
    for mode in ("420", "444"):
        files = [write(s, 1920, 1080, mode) for s in scenes]
        out["64 x 1920x1080, q80, %s" % mode] = [files[i % 8] for i in range(64)]
    base = synth.scene(256, 256, 77).reshape(256, 256, 3)
    small = []
    for i in range(64):
        w, h = 64 + (i * 37) % 193, 64 + (i * 53) % 193
        small.append(write(np.ascontiguousarray(np.roll(base, i * 5, 1)[:h, :w]).reshape(-1), w, h, ("gray", "444", "422", "420")[i % 4]))
    out["1024 x 64..256 a side, q80, all classes"] = [small[i % 64] for i in range(1024)]
    return out


def med(v):
    return "%9.2f (%8.2f)" % (statistics.median(v), min(v))


def pillow_upload(files, pool):
    arrays = list(pool.map(lambda f: np.asarray(Image.open(io.BytesIO(f))).reshape(-1), files))
    block = torch.from_numpy(np.concatenate(arrays)).cuda()
    torch.cuda.synchronize()
    return block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.load()
    lines = ["JPEG decode batch against a loop of single calls and against Pillow + one upload, %s on %s (%s)" % (
        L.pixo_hip_version().decode(), torch.cuda.get_device_name(0), socket.gethostname()),
        "Pillow %s, libjpeg-turbo %s; %d host threads for the batch and for Pillow; ms, median (min) of %d rounds after %d warm-up rounds, the forms alternating" % (
            Image.__version__, features.check_feature("libjpeg_turbo"), THREADS, ROUNDS, WARMUP),
        "call = wall time up to the synchronisation of the stream; legs: entropy decode on the host clock, the rest HIP events", ""]
    pool = ThreadPoolExecutor(THREADS)
    print("\n".join(lines), flush=True)
    for name, files in workloads().items():
        layout, total = decode.decode_jpeg_batch_info(files)
        plan = decode.decode_jpeg_batch_plan(files)
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        views = decode.decode_jpeg_batch_device(files, out=out)
        torch.cuda.synchronize()
        for k in range(0, len(files), max(len(files) // 16, 1)):
            want = np.asarray(Image.open(io.BytesIO(files[k])))
            assert views[k][0].cpu().numpy().reshape(want.shape).tobytes() == want.tobytes(), (name, k)
        t = {"batch": [], "batch one_thread": [], "loop": [], "pillow + upload": []}
        legs = []
        for r in range(WARMUP + ROUNDS):
            for form in t:
                t0 = time.perf_counter()
                if form == "batch":
                    decode.decode_jpeg_batch_device(files, out=out)
                elif form == "batch one_thread":
                    decode.decode_jpeg_batch_device(files, out=out, one_thread=True)
                elif form == "loop":
                    for f, (w, h, ct, at) in zip(files, layout):
                        decode.decode_jpeg_device(f, out=out[at:at + w * h * (int(ct) + 1)])
                else:
                    pillow_upload(files, pool)
                torch.cuda.synchronize()
                if r >= WARMUP:
                    t[form].append((time.perf_counter() - t0) * 1e3)
            ms = decode.decode_jpeg_batch_timed(files)
            if r >= WARMUP:
                legs.append(ms)
        leg = [statistics.median(x[i] for x in legs) for i in range(5)]
        # the kernel's traffic: the coefficients in (2 bytes a sample of the padded planes), the pixels out
        per_pixel = {"gray": 1.0, "444": 3.0, "422": 2.0, "420": 1.5}
        samples = sum(((w + 15) // 16 * 16) * ((h + 15) // 16 * 16) * per_pixel[cls] for (w, h, _, _), cls in zip(layout, plan["classes"]))
        moved = int(2 * samples) + total
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        copies = []
        for _ in range(WARMUP + ROUNDS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            copies.append(e0.elapsed_time(e1))
        copy_ms = statistics.median(copies[WARMUP:])
        lines.append("%s: %.1f MiB of files, %.1f MiB of pixels, %d launches, %d sub-batch(es)" % (
            name, sum(len(f) for f in files) / 2**20, total / 2**20, plan["launches"], len(plan["sub_first"]) - 1))
        lines.append("  form                          call ms")
        for form in t:
            lines.append("  %-22s %s" % (form, med(t[form])))
        lines.append("  legs of the batch (timed entry): entropy decode %.2f, uploads %.2f, kernels %.2f, copy down %.2f, whole call %.2f" % tuple(leg))
        lines.append("  kernels %.3f ms against a device copy moving the same bytes (about %.1f MiB read + written) %.3f ms: %.2f x" % (
            leg[2], moved / 2**20, copy_ms, leg[2] / copy_ms if copy_ms else 0))
        b = statistics.median(t["batch"])
        lines.append("  loop / batch: %.2f; pillow + upload / batch: %.2f; batch one_thread / batch: %.2f" % (
            statistics.median(t["loop"]) / b, statistics.median(t["pillow + upload"]) / b, statistics.median(t["batch one_thread"]) / b))
        lines.append("")
        print("\n".join(lines[-9:]), flush=True)
    text = "\n".join(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
