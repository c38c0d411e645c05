#!/usr/bin/env python3
"""How many hand-over rounds the device Huffman decode (PIXO_DECODE_DEVICE_ENTROPY) needs, from the host emulation of its
passes (tests/emu_jpeg_entropy_dec, `jpeg_entropy_main --rounds`): no GPU.  The count is the device's own — the rounds of the
launches' slowest workgroups, summed over the launches —, the number the round cap is compared with.  Over the committed decode
cases and over tests/synth.py content written by Pillow at 1920x1080.  jpeg_entropy_dec_math.h's kRoundCap is twice the largest
count in the output.

    python tools/jpeg_entropy_rounds.py [--out profiles/jpeg_entropy_rounds.txt]
"""
import argparse
import collections
import glob
import io
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from PIL import Image  # noqa: E402

import synth  # noqa: E402

EMU = os.path.join(ROOT, "tests", "emu_jpeg_entropy_dec")
W, H = 1920, 1080


def written():
    out = []
    for name, make, seeds in (("photo", synth.photo, (1, 2, 3, 4)), ("scene", synth.scene, (300, 301, 302, 303)), ("noise", synth.noise, (5, 6)),
                              ("checkerboard", lambda w, h, s: synth.checkerboard(w, h, 8), (0,)), ("gradient", lambda w, h, s: synth.gradient_rgb(w, h), (0,))):
        for seed in seeds:
            px = make(W, H, seed).reshape(H, W, 3)
            for quality, sub, tag in ((80, 2, "q80 4:2:0"), (95, 0, "q95 4:4:4"), (50, 2, "q50 4:2:0")):
                b = io.BytesIO()
                Image.fromarray(px).save(b, "JPEG", quality=quality, subsampling=sub)
                out.append(("%s, %s" % (name, tag), b.getvalue()))
            b = io.BytesIO()
            Image.fromarray(px).save(b, "JPEG", quality=80, subsampling=2, optimize=True)
            out.append(("%s, q80 4:2:0 optimised tables" % name, b.getvalue()))
    return out


def rounds_of(paths, program=None):
    rows = []
    for line in subprocess.run([program or os.path.join(EMU, "jpeg_entropy_main"), "--rounds"] + paths, stdout=subprocess.PIPE, check=True).stdout.decode().splitlines():
        f = line.split()
        rows.append(None if f[1] == "host" else {k: int(v) for k, v in (x.split("=") for x in f[1:])})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    subprocess.check_call(["make", "-C", EMU], stdout=subprocess.DEVNULL)
    geometry = dict(line.split("=") for line in subprocess.run([os.path.join(EMU, "jpeg_entropy_main"), "--geometry"], stdout=subprocess.PIPE,
                                                                  check=True).stdout.decode().split())
    lines = ["Hand-over rounds of the device Huffman decode, from the host emulation of its passes (no GPU)",
             "subsequence %s bytes, %s subsequences a workgroup, round cap %s; rounds: the launches' slowest workgroups, summed, with nothing capping them" % (
                 geometry["sub_bytes"], geometry["group_subs"], geometry["round_cap"]), ""]
    committed = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "jpeg_decode", "*.jpg")) + glob.glob(os.path.join(ROOT, "tests", "golden", "jpeg_decode_synth", "*.jpg")))
    rows = rounds_of(committed)
    dev = [r for r in rows if r]
    hist = collections.Counter(r["rounds"] for r in dev)
    lines.append("committed decode cases: %d files, %d the host's from the start, %d on the device, all vouched: %s" % (
        len(rows), len(rows) - len(dev), len(dev), all(r["vouched"] for r in dev)))
    lines.append("  rounds -> files: " + ", ".join("%d -> %d" % kv for kv in sorted(hist.items())))
    lines.append("  subsequences: up to %d; launches: up to %d" % (max(r["subs"] for r in dev), max(r["launches"] for r in dev)))
    lines.append("")
    lines.append("Pillow-written %d x %d files of tests/synth.py content:" % (W, H))
    lines.append("  %-42s %10s %6s %9s %7s %8s" % ("content", "scan bytes", "subs", "launches", "rounds", "vouched"))
    worst = max(hist)
    with tempfile.TemporaryDirectory() as d:
        files = written()
        paths = []
        for i, (_, data) in enumerate(files):
            paths.append(os.path.join(d, "%03d.jpg" % i))
            with open(paths[-1], "wb") as f:
                f.write(data)
        own = rounds_of(paths)
        for (name, _), r in zip(files, own):
            lines.append("  %-42s %10d %6d %9d %7d %8d" % (name, r["bytes"], r["subs"], r["launches"], r["rounds"], r["vouched"]))
            worst = max(worst, r["rounds"])
        # the choice of S: the same files through the emulation built with other subsequences.  A round costs a lane S bytes of
        # serial decode, so rounds x S is the serial work of the slowest file; a lane's states cost 24 bytes of HBM per S bytes.
        lines += ["", "The choice of S (the same %d files; 256 subsequences a workgroup throughout):" % len(files),
                  "  %5s %22s %22s %22s" % ("S", "largest, photo + scene", "largest, noise", "largest x S, all files")]
        for sub in (64, 128, 256):
            rows = own
            if str(sub) != geometry["sub_bytes"]:
                program = os.path.join(d, "main_%d" % sub)
                subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-O2", "-std=c++17", "-DPIXO_JE_SUB_BYTES=%d" % sub, "-o", program,
                                       os.path.join(EMU, "jpeg_entropy_main.cpp")])
                rows = rounds_of(paths, program)
            assert all(r["vouched"] for r in rows)
            calm = max(r["rounds"] for (name, _), r in zip(files, rows) if name.startswith(("photo", "scene")))
            noisy = max(r["rounds"] for (name, _), r in zip(files, rows) if name.startswith("noise"))
            lines.append("  %5d %22d %22d %22d" % (sub, calm, noisy, sub * max(r["rounds"] for r in rows)))
    lines += ["  rounds x S hardly moves: how far a lane decodes before it is in step is a property of the content in bytes (about 8 KiB in",
              "  the worst file here), so the serial work is the same at every S.  128 is chosen for what does differ: against 256 twice",
              "  the lanes to a scan (a 1080p q80 scan of 340 KB is 2,654 subsequences) and a workgroup's span of 32 KiB instead of 64 KiB",
              "  of LDS (three workgroups to a CU instead of one); against 64 half the rounds — each one a barrier, and across workgroups",
              "  a launch and a host wait — and half the lane states in HBM (24 bytes a subsequence: 19 % of the scan's bytes, not 38 %)."]
    lines += ["", "largest count at S = %s: %d; the cap is twice that: %d" % (geometry["sub_bytes"], worst, 2 * worst)]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
