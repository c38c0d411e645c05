#!/usr/bin/env python3
"""JPEG encode of images of individual sizes against a loop of single calls over the same resident images.

    python tools/jpeg_images_timing.py           -> profiles/jpeg_images_timing.txt (PIXO_TIMING_OUT=<file>: there instead)

Three sets, all resident in one block in HBM, each at 4:2:0 and 4:4:4, quality 80, baseline with the standard tables:
  (a) 64 images with sides drawn from 1280-1920 x 720-1080, RGB with every fourth one gray, photo-like (`synth.scene`) and noise
  (b) 1024 thumbnails with sides 64-256, the same mix
  (c) 64 x 1920x1080 RGB, all equal
`jpeg.encode_images_device` against a loop of `jpeg.encode_device` over the same images (the loop runs code that exists without
the images entry); on (c) also against `jpeg.encode_batch_device`, timed TWICE in every round: the difference of its two medians
is the run-to-run spread the images entry's figure on (c) is read against.  The forms alternate inside a round, every set is
warmed up first.  Written per form: host wall time around the call and the time between two HIP events recorded on the
producer stream in front of and behind it (the device's timeline of the call: kernels, copies and the gaps the host leaves
between them), median [min .. max] over the rounds, files per second, the ratio to the images entry, and the entry's plan.
No gate: the figures are what they are.
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS = 5


def bases(w, h, distinct=4):
    """(content generation is host time: a few images of the largest size, cropped)"""
    import synth
    return ([synth.scene(w, h, 100 + i).reshape(h, w, 3) for i in range(distinct)] +
            [synth.lcg_bytes(w * h * 3, 200 + i).reshape(h, w, 3) for i in range(distinct)])


def image_set(n, wr, hr, seed, gray_too=True):
    """n images with sides drawn from the ranges -> (shapes (w, h, colour type), pixels)"""
    rng = np.random.RandomState(seed)
    base = bases(wr[1], hr[1])
    shapes, pixels = [], []
    for i in range(n):
        w, h = int(rng.randint(wr[0], wr[1] + 1)), int(rng.randint(hr[0], hr[1] + 1))
        rgb = base[i % len(base)][:h, :w]
        px, ct = (rgb[:, :, 1], 0) if gray_too and i % 4 == 3 else (rgb, 2)
        shapes.append((w, h, ct))
        pixels.append(np.ascontiguousarray(px).reshape(-1))
    return shapes, pixels


def timed(fn):
    """-> (wall ms, ms between two events on the producer stream around the call)"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return (time.perf_counter() - t) * 1e3, a.elapsed_time(b)


def stats(ts, n):
    med = statistics.median(ts)
    return med, "%9.3f [%9.3f .. %9.3f] ms %9.0f files/s" % (med, min(ts), max(ts), n / med * 1e3)


def main():
    import torch
    from pixo_amd import ColorType, _lib, jpeg
    lines = ["# jpeg.encode_images_device against a loop of jpeg.encode_device over the same images in one block in HBM; per form the host",
             "# wall time around the call and the time between two HIP events around it, in ms, median [min .. max] of %d alternating" % ROUNDS,
             "# rounds after a warm-up of every form; quality 80, baseline, standard tables",
             "# device: %s (%s); torch %s, HIP %s" % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"),
                                                      torch.__version__, torch.version.hip),
             "# build: %s" % _lib.load().pixo_hip_version().decode(), ""]
    sets = [("(a) 64 images 1280-1920 x 720-1080, RGB + gray", 64, (1280, 1920), (720, 1080), True),
            ("(b) 1024 thumbnails 64-256 x 64-256, RGB + gray", 1024, (64, 256), (64, 256), True),
            ("(c) 64 x 1920x1080 RGB, all equal", 64, (1920, 1920), (1080, 1080), False)]
    for name, n, wr, hr, gray_too in sets:
        shapes, pixels = image_set(n, wr, hr, 7, gray_too)
        records, at = [], 0
        for (w, h, ct), px in zip(shapes, pixels):
            records.append((w, h, ColorType(ct), at))
            at += px.size if not gray_too else (px.size + 15) & ~15  # (c): back to back, as the batch entry takes them
        block = np.zeros(at + 16, np.uint8)
        for (_, _, _, off), px in zip(records, pixels):
            block[off:off + px.size] = px
        d_block = torch.from_numpy(block).cuda()
        views = [d_block[off:off + px.size] for (_, _, _, off), px in zip(records, pixels)]
        equal = not gray_too
        for ss in (jpeg.Subsampling.S420, jpeg.Subsampling.S444):
            o = jpeg.JpegOptions.builder(0, 0).quality(80).subsampling(ss).build()
            singles = [jpeg.JpegOptions.builder(w, h).color_type(ColorType(ct)).quality(80).subsampling(ss).build() for w, h, ct in shapes]
            forms = {"images": lambda: jpeg.encode_images_device(d_block, records, o),
                     "loop": lambda: [jpeg.encode_device(v, s) for v, s in zip(views, singles)]}
            if equal:
                forms["batch"] = lambda: jpeg.encode_batch_device(d_block, singles[0], n)
                forms["batch again"] = forms["batch"]
            got = {k: f() for k, f in forms.items()}  # the warm-up, and the files are the same
            assert all(v == got["loop"] for v in got.values()), "the forms' files differ"
            del got
            wall, events = {k: [] for k in forms}, {k: [] for k in forms}
            for _ in range(ROUNDS):
                for k, f in forms.items():
                    w_ms, e_ms = timed(f)
                    wall[k].append(w_ms)
                    events[k].append(e_ms)
            jpeg.debug_routes()
            forms["images"]()
            r = jpeg.debug_routes()
            plan = jpeg.encode_images_plan(records, o, alignment=d_block.data_ptr() % 16)
            first = len(lines)
            lines.append("%s, %s: %d sub-batch(es), %d of %d images the shared way, %d coefficient launch(es), %d coding pass(es); routes %s" %
                         (name, "4:2:0" if ss == jpeg.Subsampling.S420 else "4:4:4", len(plan["sub_first"]) - 1, sum(plan["way_in"]), n, plan["coef_launches"],
                          plan["entropy_passes"], "+".join(jpeg.route_names(r) + (["JPEG_IMAGES"] if r & jpeg.ROUTE_JPEG_IMAGES else []))))
            for what, ts in (("wall", wall), ("events", events)):
                med, text = stats(ts["images"], n)
                lines.append("    %-6s images       %s" % (what, text))
                for k in forms:
                    if k == "images":
                        continue
                    m, text = stats(ts[k], n)
                    lines.append("    %-6s %-12s %s   %s / images %.2f" % (what, k, text, k, m / med))
            if equal:
                a, b, med = statistics.median(wall["batch"]), statistics.median(wall["batch again"]), statistics.median(wall["images"])
                lines.append("    the batch entry against itself (wall): %.3f and %.3f ms, %.1f %% apart; images against the first: %+.1f %%" %
                             (a, b, abs(a - b) / min(a, b) * 100, (med - a) / a * 100))
            print("\n".join(lines[first:]), flush=True)
        del d_block, views
    out = os.path.join(ROOT, "profiles", "jpeg_images_timing.txt")
    if os.environ.get("PIXO_TIMING_OUT"):
        out = os.environ["PIXO_TIMING_OUT"]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
