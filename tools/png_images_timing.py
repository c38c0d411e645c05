#!/usr/bin/env python3
"""PNG encode of images of individual sizes against a loop of single calls over the same resident images.

    python tools/png_images_timing.py            -> profiles/png_images_timing.txt (PIXO_TIMING_OUT=<file>: there instead)

Three sets, all resident in one block in HBM, each at presets 0 and 1:
  (a) 64 images with sides drawn from 1280-1920 x 720-1080, RGB and RGBA mixed, photo-like (`synth.scene`) and noise content
  (b) 1024 thumbnails with sides 64-256, the same mix
  (c) 64 x 1920x1080 RGB, all equal
`png.encode_images_device` against a loop of `png.encode_device` over the same images (the loop runs code that exists without
the images entry); on (c) also against `png.encode_batch_device`, which is timed TWICE in every round: the difference of its
two medians is the run-to-run spread the images entry's figure on (c) is read against.  The forms alternate inside a round,
every set is warmed up first.  Written: host wall time around the call, median [min .. max] over the rounds, files per second,
the ratio to the images entry, and the entry's plan (sub-batches, images that take the shared filter launches, launches).
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


def image_set(n, wr, hr, seed, rgba_too=True):
    """n images with sides drawn from the ranges -> (shapes (w, h, colour type), pixels)"""
    rng = np.random.RandomState(seed)
    base = bases(wr[1], hr[1])
    shapes, pixels = [], []
    for i in range(n):
        w, h = int(rng.randint(wr[0], wr[1] + 1)), int(rng.randint(hr[0], hr[1] + 1))
        rgb = base[i % len(base)][:h, :w]
        if rgba_too and i % 2:
            px, ct = np.concatenate([rgb, 255 - rgb[:, :, :1] // 3], axis=2), 3
        else:
            px, ct = rgb, 2
        shapes.append((w, h, ct))
        pixels.append(np.ascontiguousarray(px).reshape(-1))
    return shapes, pixels


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def stats(ts, n):
    med = statistics.median(ts)
    return med, "%9.3f [%9.3f .. %9.3f] ms %9.0f files/s" % (med, min(ts), max(ts), n / med * 1e3)


def main():
    import torch
    from pixo_amd import ColorType, _lib, png
    lines = ["# png.encode_images_device against a loop of png.encode_device over the same images in one block in HBM; host wall time",
             "# around the call in ms, median [min .. max] of %d alternating rounds after a warm-up of every form" % ROUNDS,
             "# device: %s (%s); torch %s, HIP %s" % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"),
                                                      torch.__version__, torch.version.hip),
             "# build: %s" % _lib.load().pixo_hip_version().decode(), ""]
    sets = [("(a) 64 images 1280-1920 x 720-1080, RGB + RGBA", 64, (1280, 1920), (720, 1080), True),
            ("(b) 1024 thumbnails 64-256 x 64-256, RGB + RGBA", 1024, (64, 256), (64, 256), True),
            ("(c) 64 x 1920x1080 RGB, all equal", 64, (1920, 1920), (1080, 1080), False)]
    for name, n, wr, hr, rgba_too in sets:
        shapes, pixels = image_set(n, wr, hr, 7, rgba_too)
        records, at = [], 0
        for (w, h, ct), px in zip(shapes, pixels):
            records.append((w, h, ColorType(ct), at))
            at += (px.size + 15) & ~15
        block = np.zeros(at, np.uint8)
        for (_, _, _, off), px in zip(records, pixels):
            block[off:off + px.size] = px
        d_block = torch.from_numpy(block).cuda()
        views = [d_block[off:off + px.size] for (_, _, _, off), px in zip(records, pixels)]
        equal = not rgba_too
        for preset in (0, 1):
            o = png.PngOptions.builder(0, 0).preset(preset).build()
            singles = [png.PngOptions.builder(w, h).color_type(ColorType(ct)).preset(preset).build() for w, h, ct in shapes]
            forms = {"images": lambda: png.encode_images_device(d_block, records, o),
                     "loop": lambda: [png.encode_device(v, s) for v, s in zip(views, singles)]}
            if equal:
                forms["batch"] = lambda: png.encode_batch_device(d_block, singles[0], n)
                forms["batch again"] = forms["batch"]
            got = {k: f() for k, f in forms.items()}  # the warm-up, and the files are the same
            assert all(v == got["loop"] for v in got.values()), "the forms' files differ"
            ts = {k: [] for k in forms}
            for _ in range(ROUNDS):
                for k, f in forms.items():
                    ts[k].append(wall(f))
            plan = png.encode_images_plan(records, o, alignment=d_block.data_ptr() % 16)
            med, text = stats(ts["images"], n)
            lines.append("%s, preset %d: %d sub-batch(es), %d of %d images through %d shared filter launch(es)" %
                         (name, preset, len(plan["sub_first"]) - 1, sum(plan["way_in"]), n, plan["filter_launches"]))
            lines.append("    images       %s" % text)
            for k in forms:
                if k == "images":
                    continue
                m, text = stats(ts[k], n)
                lines.append("    %-12s %s   %s / images %.2f" % (k, text, k, m / med))
            if equal:
                a, b = statistics.median(ts["batch"]), statistics.median(ts["batch again"])
                lines.append("    the batch entry against itself: %.3f and %.3f ms, %.1f %% apart; images against the first: %+.1f %%" %
                             (a, b, abs(a - b) / min(a, b) * 100, (med - a) / a * 100))
            print("\n".join(lines[-6:]), flush=True)
        del d_block, views
    out = os.path.join(ROOT, "profiles", "png_images_timing.txt")
    if os.environ.get("PIXO_TIMING_OUT"):
        out = os.environ["PIXO_TIMING_OUT"]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
