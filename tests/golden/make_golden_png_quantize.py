#!/usr/bin/env python3
"""Generate the PNG lossy-mode vectors with the REFERENCE's own code.

Runs `encodePng(..., lossy = true)` of the reference's compiled WebAssembly build (oracle/_ref/pixo_bg.wasm) under node via
oracle/ref_wasm.js on deterministic inputs: Auto quantisation, 256 colours, dithering on (src/png/mod.rs:203-213) — the one
setting the wasm reaches.  Per case it records the generator parameters, whether the reference wrote the indexed file
(`applied`: the gate fired; read from the reference's file, and the model's gate must agree), the reference's file length, every chunk that is not IDAT (hex), the two zlib header bytes, the
Adler-32 trailer, length and sha256 of the inflated IDAT, the IDAT body lengths.  The reference's files themselves are kept
under tests/golden/png_quantize/ only where they are a few KB.  Build container only (needs node + the staged wasm).

    python tests/golden/make_golden_png_quantize.py
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
    import synth
    w, h, ct, gen, seed = c["w"], c["h"], c["color_type"], c["gen"], c["seed"]
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    if gen == "pal":  # n random colours over a smooth index field; RGBA: about 30 % of the entries are not opaque
        n = c["n"]
        pal = synth.lcg_bytes(n * 4, seed).reshape(n, 4).copy()
        pal[:, 0] = (np.arange(n) * 7) & 255  # (r, g) differ for every entry below 65,536: n distinct colours
        pal[:, 1] = ((np.arange(n) * 7) >> 8) * 37 & 255
        pal[pal[:, 3] % 10 >= 3, 3] = 255
        wobble = synth.lcg_bytes(w * h, seed + 1).reshape(h, w) % 3
        idx = ((x * 5 + y * 3) * (n + 8) // (5 * (w - 1) + 3 * (h - 1) + 1) + wobble) % n  # (wraps a little: the sparse corners still reach every entry)
        px = pal[idx]
        return np.ascontiguousarray(px if ct == 3 else px[:, :, :3]).reshape(-1)
    if gen in ("photo4", "scene4"):  # every channel masked to its top 4 bits: at most 4,096 colours (RGBA: one other alpha)
        rgb = (synth.photo(w, h, seed) if gen == "photo4" else synth.scene(w, h, seed)).reshape(h, w, 3) & 0xF0
        if ct == 2:
            return np.ascontiguousarray(rgb).reshape(-1)
        alpha = np.where((x * 7 + y * 3) % 10 >= 3, 255, 0x80).astype(np.uint8)
        return np.concatenate([rgb, alpha[:, :, None]], axis=2).reshape(-1)
    if gen == "many":  # far more than 32 * 256 sampled colours: Auto declines
        v = (x.astype(np.uint32) + w * y).astype(np.uint32) * 2654435761 >> 8
        rgb = np.stack(np.broadcast_arrays(v & 255, (v >> 8) & 255, (v >> 16) & 255), axis=2).astype(np.uint8)
        return (rgb if ct == 2 else np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], axis=2)).reshape(-1)
    if gen == "noise":  # gray inputs: never quantised
        b = synth.lcg_bytes(w * h * BPP[ct], seed)
        if ct == 1:
            b[1::2] |= 1
        return b
    raise ValueError(c)


def cases():
    cs = []

    def add(gen, w, h, ct, preset, seed=1, **kw):
        tag = "_".join("%s%s" % (k[0], v) for k, v in sorted(kw.items()))
        cs.append(dict(gen=gen, w=w, h=h, color_type=ct, preset=preset, seed=seed,
                       name="%s%s_%dx%d_c%d_p%d" % (gen, "_" + tag if tag else "", w, h, ct, preset), **kw))

    for n, preset in ((257, 1), (300, 0), (1000, 2), (4000, 1)):
        add("pal", 130, 65, 2, preset, seed=10 + n % 7, n=n)       # band boundary at 64 rows
    add("pal", 5, 200, 2, 0, seed=3, n=300)                        # rows finish before the band's last lanes start
    add("pal", 67, 129, 3, 1, seed=4, n=1000)                      # band boundaries at 64 and 128 rows
    add("pal", 257, 131, 3, 2, seed=5, n=1000)                     # the direct search inside the chain
    add("pal", 317, 317, 2, 1, seed=6, n=4000)                     # strides 5 / 2
    add("pal", 512, 512, 3, 0, seed=7, n=1000)                     # strides 13 / 5
    add("pal", 64, 48, 2, 1, seed=8, n=1000)
    add("pal", 64, 48, 3, 1, seed=9, n=300)
    add("photo4", 130, 65, 2, 1, seed=42)
    add("photo4", 512, 512, 2, 1, seed=42)
    add("scene4", 67, 129, 3, 2, seed=42)
    add("scene4", 130, 65, 3, 0, seed=42)
    # Auto declines: too few colours, exactly max_colors, too many, gray inputs
    add("pal", 130, 65, 2, 1, seed=20, n=100)
    add("pal", 130, 65, 3, 0, seed=21, n=256)
    add("many", 300, 200, 2, 0)
    add("noise", 64, 48, 0, 1, seed=22)
    add("noise", 64, 48, 1, 1, seed=23)
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


def sampled_colours(c):
    """distinct colours among the gate's and among the histogram's samples"""
    import png_quantize_model as M
    keys = M.keys_of(make_input(c), BPP[c["color_type"]])
    n = len(keys)
    return len(np.unique(keys[::max(n // 20000, 1)])), len(np.unique(keys[::max(n // 50000, 1)]))


def main():
    import png_quantize_model as M
    cs = cases()
    assert len({c["name"] for c in cs}) == len(cs)
    os.makedirs(os.path.join(HERE, "png_quantize"), exist_ok=True)
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        man = {"cases": []}
        for k, c in enumerate(cs):
            inp = os.path.join(tmp, "in%d.bin" % k)
            make_input(c).tofile(inp)
            man["cases"].append(dict(kind="png", input=inp, w=c["w"], h=c["h"], color_type=c["color_type"], preset=c["preset"],
                                     lossy=True, output=os.path.join(tmp, "out%d.png" % k)))
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
            spp = BPP[c["color_type"]]
            # Whether the REFERENCE quantised, read from its file: an 8-bit palette image whose rows are all unfiltered, from an
            # input the lossless path could not have turned into a palette (more than 256 colours, or preset 0: no reduce_palette)
            keys = M.keys_of(make_input(c), spp) if spp >= 3 else None
            lossless_palette = spp >= 3 and c["preset"] != 0 and len(np.unique(keys)) <= 256
            indexed = other[0][1][8:10] == b"\x08\x03" and len(stream) == c["h"] * (c["w"] + 1) and not any(stream[::c["w"] + 1])
            applied = indexed and not lossless_palette
            assert not (indexed and lossless_palette) or len(other[1][1]) // 3 == len(np.unique(keys)), c["name"]  # (then it IS the lossless palette)
            assert M.should_quantize(M.AUTO, spp, keys, 256) == applied, (c["name"], "the model's gate disagrees with the reference")
            if applied:  # Auto must fire under BOTH strides, and the 8,192 cut (the one open point of the source) must stay out
                g, hs = sampled_colours(c)
                assert 257 <= g <= 8192 and 257 <= hs <= 8192, (c["name"], g, hs)
            rec = dict(c, applied=bool(applied), ref_len=len(png), chunks=[[t, b.hex()] for t, b in other], zlib_header=z[:2].hex(),
                       adler32=struct.unpack(">I", z[-4:])[0], stream_len=len(stream), stream_sha256=hashlib.sha256(stream).hexdigest(),
                       idat_lens=[len(b) for b in idat])
            assert rec["adler32"] == zlib.adler32(stream)
            if len(png) <= STORE_LIMIT:
                open(os.path.join(HERE, "png_quantize", c["name"] + ".png"), "wb").write(png)
                rec["stored"] = True
            out.append(rec)
            print(c["name"], "applied" if applied else "declined", len(png), [t for t, _ in other], z[:2].hex(), "%.0f ms" % r["ms"][0])
    json.dump({"wasm_sha256": hashlib.sha256(open(os.path.join(ROOT, "oracle", "_ref", "pixo_bg.wasm"), "rb").read()).hexdigest(),
               "cases": out}, open(os.path.join(HERE, "png_quantize_cases.json"), "w"), indent=0)


if __name__ == "__main__":
    main()
