#!/usr/bin/env python3
"""PNG whole files on the device: sizes against the reference, and where the time goes.

    python tools/png_encode_timing.py sizes     -> profiles/png_encode_sizes.txt
    python tools/png_encode_timing.py timing    -> profiles/png_encode_timing.txt

sizes: every case of tests/golden/png_files.json encoded by `png.encode`; device file length / reference file length at
the same preset (both compress the same prepared stream, so the ratio isolates DEFLATE), and the largest ratio per content
class and preset — the numbers behind SIZE_BOUNDS in tests/test_gpu_png_encode.py.

timing: 4096 x 4096 RGBA and RGB on gradient, photo-like and noise content, preset 0.  Device events around repeated
calls (median [min .. max]): the whole `encode_device` call, `prepare_device` alone, the device zlib stage alone
(`zlib_compress_device` on the prepared stream: chunk kernel + scan + compaction and the one host decision between them),
and beside them what a caller did before this path existed: `prepare_device`, the stream copied to the host,
`zlib.compress(stream, 1)` on one core.
"""
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sizes(path):
    import png_file_cases as PF
    from pixo_amd import png
    worst = {}
    with open(path, "w") as f:
        f.write("# device file length / reference file length, same preset, same prepared stream (tests/golden/png_files.json)\n")
        f.write("# preset 2 is Zopfli-style in the reference: recorded, no bound\n")
        f.write("%-40s %-6s %6s %10s %10s %8s\n" % ("case", "class", "preset", "device", "reference", "ratio"))
        for c in PF.CASES:
            n = len(png.encode(PF.make_input(c), PF.options(c)))
            r = n / c["ref_len"]
            f.write("%-40s %-6s %6d %10d %10d %8.4f\n" % (c["name"], c["kind"], c["preset"], n, c["ref_len"], r))
            key = (c["kind"], c["preset"])
            worst[key] = max(worst.get(key, 0.0), r)
        f.write("\n# largest ratio per class and preset\n")
        for (kind, preset), r in sorted(worst.items()):
            f.write("%-6s preset %d  %.4f\n" % (kind, preset, r))
    print(open(path).read())


def timed(fn, reps):
    import torch
    fn()
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return "%9.3f [%.3f .. %.3f] ms" % (ms[len(ms) // 2], ms[0], ms[-1])


def timing(path, side=4096, reps=7):
    import torch
    import synth
    from pixo_amd import ColorType, png
    w = h = side
    with open(path, "w") as f:
        f.write("# PNG whole-file path, %dx%d, preset 0; %s; %d timed calls after 2 warm-up calls, device events around each call\n"
                % (w, h, torch.cuda.get_device_name(0), reps))
        tile = 512
        contents = {
            "gradient": lambda: synth.gradient_rgb(w, h).reshape(h, w, 3),
            "photo-like": lambda: np.tile(synth.photo(tile, tile, 42).reshape(tile, tile, 3), (h // tile, w // tile, 1))
            + (np.arange(w)[None, :, None] // tile + np.arange(h)[:, None, None] // tile).astype(np.uint8),  # tiles differ by a constant
            "noise": lambda: synth.lcg_bytes(w * h * 3, 5).reshape(h, w, 3),
        }
        for name, make in contents.items():
            rgb = np.ascontiguousarray(make().astype(np.uint8))
            for ct in (ColorType.Rgba, ColorType.Rgb):
                px = rgb if ct == ColorType.Rgb else np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], axis=2)
                o = png.PngOptions.builder(w, h).color_type(ct).preset(0).build()
                d_px = torch.from_numpy(px.reshape(-1)).cuda()
                d_stream = torch.empty(o.full_size(), dtype=torch.uint8, device="cuda")
                n, lay, _ = png.prepare_device(d_px, o, d_stream)
                cap = png.stored_bound(n)
                d_z = torch.empty(cap, dtype=torch.uint8, device="cuda")
                file_len = len(png.encode_device(d_px, o))
                zlen = png.zlib_compress_device(d_stream, n, d_z, cap, bpp=lay.bytes_per_pixel, row=lay.row_bytes + 1)
                f.write("\n## %s, %s: stream %d bytes, file %d bytes (zlib stream %d)\n" % (name, ct.name, n, file_len, zlen))
                f.write("encode_device, whole call             %s\n" % timed(lambda: png.encode_device(d_px, o), reps))
                f.write("prepare_device alone                  %s\n" % timed(lambda: png.prepare_device(d_px, o, d_stream), reps))
                f.write("device zlib stage alone               %s\n" % timed(
                    lambda: png.zlib_compress_device(d_stream, n, d_z, cap, bpp=lay.bytes_per_pixel, row=lay.row_bytes + 1), reps))
                t0 = time.perf_counter()
                png.prepare_device(d_px, o, d_stream)
                host = d_stream[:n].cpu().numpy()
                t1 = time.perf_counter()
                ref = zlib.compress(host, 1)
                t2 = time.perf_counter()
                f.write("before: prepare_device + copy to host %9.3f ms, zlib.compress(stream, 1) on one core %9.1f ms -> %d bytes\n"
                        % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, len(ref)))
                f.flush()
    print(open(path).read())


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "sizes"
    if what == "sizes":
        sizes(os.path.join(ROOT, "profiles", "png_encode_sizes.txt"))
    else:
        timing(os.path.join(ROOT, "profiles", "png_encode_timing.txt"), *(int(a) for a in sys.argv[2:3]))
