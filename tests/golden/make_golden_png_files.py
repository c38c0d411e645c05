#!/usr/bin/env python3
"""Generate the whole-file PNG vectors with the REFERENCE's own code.

Runs `encodePng` of the reference's compiled WebAssembly build (oracle/_ref/pixo_bg.wasm) under node via
oracle/ref_wasm.js on deterministic inputs and records, per case, what a file of this library must reproduce and what it
is measured against: the generator parameters, the reference's file length, every chunk that is not IDAT (hex), the two
zlib header bytes, the Adler-32 trailer, length and sha256 of the inflated IDAT (the prepared stream), the IDAT body
lengths.  The reference's files themselves are kept under tests/golden/png_files/ only where they are a few KB.  Build
container only (needs node + the staged wasm).

    python tests/golden/make_golden_png_files.py
"""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

STORE_LIMIT = 8192
BPP = {0: 1, 1: 2, 2: 3, 3: 4}


def make_input(c):
    """The pixels of a case, from its parameters alone."""
    import make_golden_png_reduce as MR
    import synth
    w, h, ct, gen, seed = c["w"], c["h"], c["color_type"], c["gen"], c["seed"]
    if gen == "noise":
        b = synth.lcg_bytes(w * h * BPP[ct], seed)
        if ct in (1, 3):
            b[BPP[ct] - 1::BPP[ct]] |= 1  # no alpha 0: optimize_alpha would change the pixels
        return b
    if gen in ("gradient", "photo", "scene"):
        rgb = (synth.gradient_rgb(w, h) if gen == "gradient" else synth.photo(w, h, seed) if gen == "photo" else synth.scene(w, h, seed)).reshape(h, w, 3)
        alpha = (255 - (np.arange(w)[None, :] + np.arange(h)[:, None]) * 127 // (w + h)).astype(np.uint8)
        if ct == 0:
            return np.ascontiguousarray(rgb[:, :, 0]).reshape(-1)
        if ct == 1:
            return np.stack([rgb[:, :, 0], alpha], axis=2).reshape(-1)
        if ct == 2:
            return np.ascontiguousarray(rgb).reshape(-1)
        return np.concatenate([rgb, alpha[:, :, None]], axis=2).reshape(-1)
    if gen == "flat":  # four colours: a 2-bit palette at presets 1 and 2
        rgb = synth.flat_blocks(w, h).reshape(h, w, 3)
        return (rgb if ct == 2 else np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], axis=2)).reshape(-1)
    if gen in ("pal", "grays"):
        return MR.make_input(c)
    raise ValueError(c)


def cases():
    cs = []

    def add(gen, kind, w, h, ct, preset, seed=1, **kw):
        tag = "_".join("%s%s" % (k[0], v) for k, v in sorted(kw.items()))
        cs.append(dict(gen=gen, kind=kind, w=w, h=h, color_type=ct, preset=preset, seed=seed,
                       name="%s%s_%dx%d_c%d_p%d" % (gen, "_" + tag if tag else "", w, h, ct, preset), **kw))

    for ct in (0, 1, 2, 3):  # all four colour types at presets 0, 1 and 2
        for preset in (0, 1, 2):
            add("noise", "noise", 61, 47, ct, preset, seed=3 + ct)
            add("gradient", "flat", 128, 96, ct, preset)
    for preset in (0, 1, 2):
        add("flat", "flat", 96, 64, 2, preset)
        add("flat", "flat", 96, 64, 3, preset)
    for preset in (1, 2):  # <= 256 colours: a palette with tRNS
        add("pal", "low", 90, 75, 3, preset, seed=5, n=13, alpha="some", pattern="popular")
        add("pal", "low", 71, 67, 3, preset, seed=6, n=200, alpha="some", pattern="noise")
    for n in (2, 4, 16):       # gray pixels that drop to 1, 2 and 4 bits (as a palette of grays: the reference's choice)
        add("grays", "low", 97, 53, 2, 1, seed=7 + n, n=n)
    add("grays", "low", 97, 53, 3, 2, seed=30, n=4)
    for gen in ("photo", "scene"):
        for ct in (2, 3):
            for preset in (0, 1):
                add(gen, "photo", 512, 512, ct, preset, seed=42)
        add(gen, "photo", 128, 96, 2, 2, seed=42)
    add("noise", "noise", 300, 300, 3, 0, seed=9)  # two IDAT chunks
    add("gradient", "flat", 512, 512, 3, 0)
    add("gradient", "flat", 512, 512, 2, 1)
    return cs


def parse_png(png):
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    i, idat, other = 8, [], []
    while i < len(png):
        n, typ = struct.unpack(">I4s", png[i:i + 8])
        body = png[i + 8:i + 8 + n]
        assert struct.unpack(">I", png[i + 8 + n:i + 12 + n])[0] == zlib.crc32(typ + body)
        if typ == b"IDAT":
            idat.append(body)
        else:
            other.append((typ.decode(), body))
        i += 12 + n
    assert i == len(png)
    return idat, other


def main():
    cs = cases()
    assert len({c["name"] for c in cs}) == len(cs)
    os.makedirs(os.path.join(HERE, "png_files"), exist_ok=True)
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        man = {"cases": []}
        for k, c in enumerate(cs):
            inp = os.path.join(tmp, "in%d.bin" % k)
            make_input(c).tofile(inp)
            man["cases"].append(dict(kind="png", input=inp, w=c["w"], h=c["h"], color_type=c["color_type"], preset=c["preset"],
                                     lossy=False, output=os.path.join(tmp, "out%d.png" % k)))
        mp = os.path.join(tmp, "manifest.json")
        json.dump(man, open(mp, "w"))
        res = subprocess.run(["node", "--max-old-space-size=4096", os.path.join(ROOT, "oracle", "ref_wasm.js"), mp],
                             stdout=subprocess.PIPE, check=True).stdout.decode().strip().splitlines()
        for k, (c, line) in enumerate(zip(cs, res)):
            r = json.loads(line)
            assert r["ok"], (c, r)
            png = open(man["cases"][k]["output"], "rb").read()
            idat, other = parse_png(png)
            z = b"".join(idat)
            stream = zlib.decompress(z)
            assert all(len(b) == 262144 for b in idat[:-1])
            rec = dict(c, ref_len=len(png), chunks=[[t, b.hex()] for t, b in other], zlib_header=z[:2].hex(), adler32=struct.unpack(">I", z[-4:])[0],
                       stream_len=len(stream), stream_sha256=hashlib.sha256(stream).hexdigest(), idat_lens=[len(b) for b in idat])
            assert rec["adler32"] == zlib.adler32(stream)
            if len(png) <= STORE_LIMIT:
                open(os.path.join(HERE, "png_files", c["name"] + ".png"), "wb").write(png)
                rec["stored"] = True
            out.append(rec)
            print(c["name"], len(png), [t for t, _ in other], z[:2].hex())
    json.dump({"wasm_sha256": hashlib.sha256(open(os.path.join(ROOT, "oracle", "_ref", "pixo_bg.wasm"), "rb").read()).hexdigest(),
               "cases": out}, open(os.path.join(HERE, "png_files.json"), "w"), indent=0)


if __name__ == "__main__":
    main()
