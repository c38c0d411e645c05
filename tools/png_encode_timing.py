#!/usr/bin/env python3
"""PNG whole files on the device: sizes against the reference, and where the time goes.

    python tools/png_encode_timing.py sizes     -> profiles/png_encode_sizes.txt
    python tools/png_encode_timing.py timing    -> profiles/png_encode_timing.txt

sizes: every case of tests/golden/png_files.json encoded by `png.encode` at both efforts of the device DEFLATE (the default,
and `flags=png.EFFORT_HIGH`); device file length / reference file length at the same preset (both compress the same
prepared stream, so the ratio isolates DEFLATE), and the largest ratio per content class, preset and effort — the numbers
behind SIZE_BOUNDS in tests/test_gpu_png_encode.py and tests/test_gpu_png_deflate_effort.py.

timing: 4096 x 4096 RGBA and RGB on gradient, photo-like and noise content, preset 0.  Device events around repeated
calls (median [min .. max]): the whole `encode_device` call, `prepare_device` alone, the device zlib stage alone
(`zlib_compress_device` on the prepared stream: one unframed segment through the tail — chunk kernel, the checksum joined
on the host from the chunks' records, scan + compaction),
and beside them what a caller did before this path existed: `prepare_device`, the stream copied to the host,
`zlib.compress(stream, 1)` on one core.  Every device row is given at both efforts, the high one also as a ratio to the
default of the same call.  Behind them, each in a fresh child process per library (PIXO_HIP_LIB):
  - the S x K table: for every tools/ab/ab_effort_s<S>_k<K>.so (tools/ab_build.sh with -DPIXO_PNG_EFFORT_SUBSTEP=<S>
    -DPIXO_PNG_EFFORT_PROBES=<K>, AB_SRC="png_deflate.hip png_encode_api.cpp") the flagged sizes of the gradient fixtures and
    the zlib stage's time on the 4096 x 4096 RGB gradient — what kZEffortSubstep / kZEffortProbes were chosen from;
  - the A/B of the default effort: tools/ab/ab_parent.so (AB_REV=<parent> tools/ab_build.sh parent) against the in-tree
    library, alternating, through the entry both have (pixo_hip_zlib_compress_device).
"""
import ctypes
import glob
import os
import re
import subprocess
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
        f.write("# default: the options of the fixture; high: the same with flags |= png.EFFORT_HIGH (sub-steps of %d, %d chain entries)\n"
                % png.deflate_effort_params())
        f.write("%-40s %-6s %6s %10s %10s %10s %8s %8s\n" % ("case", "class", "preset", "default", "high", "reference", "ratio", "high"))
        for c in PF.CASES:
            o = PF.options(c)
            n = len(png.encode(PF.make_input(c), o))
            o.flags |= png.EFFORT_HIGH
            m = len(png.encode(PF.make_input(c), o))
            r, rh = n / c["ref_len"], m / c["ref_len"]
            f.write("%-40s %-6s %6d %10d %10d %10d %8.4f %8.4f\n" % (c["name"], c["kind"], c["preset"], n, m, c["ref_len"], r, rh))
            key = (c["kind"], c["preset"])
            worst[key] = (max(worst.get(key, (0.0, 0.0))[0], r), max(worst.get(key, (0.0, 0.0))[1], rh))
        f.write("\n# largest ratio per class and preset: default, high\n")
        for (kind, preset), (r, rh) in sorted(worst.items()):
            f.write("%-6s preset %d  %.4f  %.4f\n" % (kind, preset, r, rh))
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
    return "%9.3f [%.3f .. %.3f] ms" % (ms[len(ms) // 2], ms[0], ms[-1]), ms[len(ms) // 2]


def contents(w, h):
    import synth
    tile = 512
    return {
        "gradient": lambda: synth.gradient_rgb(w, h).reshape(h, w, 3),
        "photo-like": lambda: np.tile(synth.photo(tile, tile, 42).reshape(tile, tile, 3), (h // tile, w // tile, 1))
        + (np.arange(w)[None, :, None] // tile + np.arange(h)[:, None, None] // tile).astype(np.uint8),  # tiles differ by a constant
        "noise": lambda: synth.lcg_bytes(w * h * 3, 5).reshape(h, w, 3),
    }


def prepared(rgb, w, h):
    """-> (device stream, its length, bpp hint, row hint, device output, its capacity) of an RGB image at preset 0"""
    import torch
    from pixo_amd import ColorType, png
    o = png.PngOptions.builder(w, h).color_type(ColorType.Rgb).preset(0).build()
    d_px = torch.from_numpy(np.ascontiguousarray(rgb.astype(np.uint8)).reshape(-1)).cuda()
    d_stream = torch.empty(o.full_size(), dtype=torch.uint8, device="cuda")
    n, lay, _ = png.prepare_device(d_px, o, d_stream)
    cap = png.stored_bound(n)
    return d_stream, n, lay.bytes_per_pixel, lay.row_bytes + 1, torch.empty(cap, dtype=torch.uint8, device="cuda"), cap


def grid_child(side, reps):
    """One line for the library PIXO_HIP_LIB names: its constants, the flagged gradient fixtures, the 4096^2 gradient."""
    import png_file_cases as PF
    from pixo_amd import png
    s, k = png.deflate_effort_params()
    total, named = 0, []
    for c in PF.CASES:
        if c["gen"] == "gradient" and c["preset"] in (0, 1):
            o = PF.options(c)
            o.flags |= png.EFFORT_HIGH
            n = len(png.encode(PF.make_input(c), o))
            total += n
            if c["name"] in ("gradient_128x96_c3_p1", "gradient_128x96_c1_p0", "gradient_128x96_c2_p1", "gradient_512x512_c3_p0"):
                named.append(n)
    d_stream, n, bpp, row, d_z, cap = prepared(contents(side, side)["gradient"](), side, side)
    zlen = png.zlib_compress_device(d_stream, n, d_z, cap, bpp=bpp, row=row, effort=1)
    t, _ = timed(lambda: png.zlib_compress_device(d_stream, n, d_z, cap, bpp=bpp, row=row, effort=1), reps)
    print("GRID S %3d K %d  gradient fixtures, presets 0 and 1: %6d bytes (c3_p1 %d, c1_p0 %d, c2_p1 %d, 512x512_c3_p0 %d)  %dx%d gradient: %8d bytes %s"
          % ((s, k, total) + tuple(named) + (side, side, zlen, t)))


def ab_child(side, reps):
    """The default effort through pixo_hip_zlib_compress_device, the entry every build has."""
    from pixo_amd import _lib
    L = _lib.load()
    for name, make in contents(side, side).items():
        d_stream, n, bpp, row, d_z, cap = prepared(make(), side, side)
        out = ctypes.c_size_t()

        def call():
            _lib.check(L.pixo_hip_zlib_compress_device(d_stream.data_ptr(), n, 6, bpp, row, d_z.data_ptr(), cap, ctypes.byref(out)))
        t, _ = timed(call, reps)
        print("AB %-12s %-10s default effort, zlib stage: %8d bytes %s" % (os.path.basename(_lib.LIB_PATH), name, out.value, t))


def children(f, mode, libs, side, reps):
    """Runs `mode` once per library in a fresh process and copies its lines; stops at the first child that does not end well."""
    for lib in libs:
        env = dict(os.environ)
        if lib:
            env["PIXO_HIP_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, str(side), str(reps)], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, universal_newlines=True, timeout=240)
        lines = [l for l in r.stdout.splitlines() if l.startswith(("GRID", "AB"))]
        f.write("".join(re.sub(r"^(GRID|AB) ", "", l) + "\n" for l in lines))
        f.flush()
        print("\n".join(lines), flush=True)
        if r.returncode:
            f.write("# %s %s ended with status %d:\n%s\n" % (mode, lib, r.returncode, r.stdout[-2000:]))
            raise SystemExit("%s %s ended with status %d" % (mode, lib, r.returncode))


def timing(path, side=4096, reps=7):
    import torch
    from pixo_amd import ColorType, png
    w = h = side
    with open(path, "w") as f:
        f.write("# PNG whole-file path, %dx%d, preset 0; %s; %d timed calls after 2 warm-up calls, device events around each call\n"
                % (w, h, torch.cuda.get_device_name(0), reps))
        f.write("# high: flags |= png.EFFORT_HIGH / effort=1 (sub-steps of %d, %d chain entries); its ratio is to the default row above it\n"
                % png.deflate_effort_params())
        for name, make in contents(w, h).items():
            rgb = np.ascontiguousarray(make().astype(np.uint8))
            for ct in (ColorType.Rgba, ColorType.Rgb):
                px = rgb if ct == ColorType.Rgb else np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], axis=2)
                o = png.PngOptions.builder(w, h).color_type(ct).preset(0).build()
                oh = png.PngOptions.builder(w, h).color_type(ct).preset(0).flags(png.EFFORT_HIGH).build()
                d_px = torch.from_numpy(px.reshape(-1)).cuda()
                d_stream = torch.empty(o.full_size(), dtype=torch.uint8, device="cuda")
                n, lay, _ = png.prepare_device(d_px, o, d_stream)
                cap = png.stored_bound(n)
                d_z = torch.empty(cap, dtype=torch.uint8, device="cuda")
                file_len = len(png.encode_device(d_px, o))
                zlen = png.zlib_compress_device(d_stream, n, d_z, cap, bpp=lay.bytes_per_pixel, row=lay.row_bytes + 1)
                f.write("\n## %s, %s: stream %d bytes, file %d bytes (zlib stream %d)\n" % (name, ct.name, n, file_len, zlen))
                print("timing %s %s" % (name, ct.name), flush=True)
                t, whole = timed(lambda: png.encode_device(d_px, o), reps)
                f.write("encode_device, whole call             %s\n" % t)
                f.write("prepare_device alone                  %s\n" % timed(lambda: png.prepare_device(d_px, o, d_stream), reps)[0])
                t, stage = timed(lambda: png.zlib_compress_device(d_stream, n, d_z, cap, bpp=lay.bytes_per_pixel, row=lay.row_bytes + 1), reps)
                f.write("device zlib stage alone               %s\n" % t)
                file_high = len(png.encode_device(d_px, oh))
                zhigh = png.zlib_compress_device(d_stream, n, d_z, cap, bpp=lay.bytes_per_pixel, row=lay.row_bytes + 1, effort=1)
                f.write("high: file %d bytes (zlib stream %d), %.4f of the default's\n" % (file_high, zhigh, file_high / file_len))
                t, ms = timed(lambda: png.encode_device(d_px, oh), reps)
                f.write("high: encode_device, whole call       %s  x %.2f\n" % (t, ms / whole))
                t, ms = timed(lambda: png.zlib_compress_device(d_stream, n, d_z, cap, bpp=lay.bytes_per_pixel, row=lay.row_bytes + 1, effort=1), reps)
                f.write("high: device zlib stage alone         %s  x %.2f\n" % (t, ms / stage))
                t0 = time.perf_counter()
                png.prepare_device(d_px, o, d_stream)
                host = d_stream[:n].cpu().numpy()
                t1 = time.perf_counter()
                ref = zlib.compress(host, 1)
                t2 = time.perf_counter()
                f.write("before: prepare_device + copy to host %9.3f ms, zlib.compress(stream, 1) on one core %9.1f ms -> %d bytes\n"
                        % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, len(ref)))
                f.flush()
        ab = os.path.join(ROOT, "tools", "ab")
        grid = sorted(glob.glob(os.path.join(ab, "ab_effort_s*_k*.so")))
        if grid:
            f.write("\n## the S x K table: sub-step of the links x chain entries tried; RGB gradient, zlib stage alone, effort 1, a fresh process per build\n")
            children(f, "grid-child", grid, side, reps)
        parent = os.path.join(ab, "ab_parent.so")
        if os.path.exists(parent):
            f.write("\n## A/B of the default effort: the parent commit's library (ab_parent.so) against this tree's, alternating, a fresh process each; RGB\n")
            children(f, "ab-child", [parent, "", parent, ""], side, reps)
    print(open(path).read())


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "sizes"
    if what == "sizes":
        sizes(os.path.join(ROOT, "profiles", "png_encode_sizes.txt"))
    elif what in ("grid-child", "ab-child"):
        (grid_child if what == "grid-child" else ab_child)(int(sys.argv[2]), int(sys.argv[3]))
    else:
        timing(os.path.join(ROOT, "profiles", "png_encode_timing.txt"), *(int(a) for a in sys.argv[2:3]))
