#!/usr/bin/env python3
"""Generate the vectors of the PNG reductions with the REFERENCE's own code.

Runs `encodePng` of the reference's compiled WebAssembly build (oracle/_ref/pixo_bg.wasm) under node via
oracle/ref_wasm.js on deterministic inputs chosen to reach the branches of maybe_reduce_color_type and
maybe_optimize_alpha (src/png/mod.rs:633-836): palettes at 1/2/4/8 bits with and without tRNS, RGBA -> RGB, RGBA ->
GrayAlpha, RGBA kept with transparent pixels, GrayAlpha and Gray inputs.  Parses the PNG, inflates IDAT and records per
case: IHDR bit depth / colour type, PLTE and tRNS bytes, the filter byte of every row, length / sha256 / Adler-32 of the
prepared stream; streams of at most 24,000 bytes are stored verbatim under tests/golden/png_reduce/.  Every case names
the branch it is meant to take (`expect`) and the generator asserts that the reference took it.  Build container only
(needs node + the staged wasm).

    python tests/golden/make_golden_png_reduce.py [--huge]     # --huge adds the 4096x4096 case
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

STORE_LIMIT = 24000
BPP = {0: 1, 1: 2, 2: 3, 3: 4}


def palette_colors(n, alpha, rng):
    """n distinct RGBA colours.  alpha: 'opaque' | 'some' (a few alphas != 255) | 'zero' (also alpha 0 with different rgb)"""
    seen, out = set(), []
    while len(out) < n:
        c = tuple(int(v) for v in rng.randint(0, 256, 3))
        if c not in seen:
            seen.add(c)
            out.append(c)
    a = np.full(n, 255, np.int64)
    if alpha in ("some", "zero"):
        a[::3] = rng.randint(1, 255, len(a[::3]))
    if alpha == "zero":
        a[:max(2, n // 4)] = 0
    return np.array([c + (int(x),) for c, x in zip(out, a)], np.uint8)


def index_image(w, h, n, pattern, rng):
    y, x = np.mgrid[0:h, 0:w]
    if pattern == "noise":
        return rng.randint(0, n, (h, w))
    if pattern == "smooth":       # diagonal bands: every colour equally frequent
        return ((x // max(1, w // (2 * n) or 1) + y // max(1, h // n or 1)) % n)
    if pattern == "popular":      # one background colour, the others in noisy patches
        img = np.zeros((h, w), np.int64)
        m = rng.rand(h, w) < 0.35
        img[m] = rng.randint(0, n, int(m.sum()))
        return img
    if pattern == "popular_last":  # the background is the last sorted key
        img = np.full((h, w), n - 1, np.int64)
        m = ((x * 7 + y * 3) % 5) == 0
        img[m] = ((x + y) % n)[m]
        return img
    raise ValueError(pattern)


def make_input(c):
    w, h, ct, gen, seed = c["w"], c["h"], c["color_type"], c["gen"], c["seed"]
    rng = np.random.RandomState(seed)
    if gen == "pal":
        cols = palette_colors(c["n"], c["alpha"], rng)
        order = np.lexsort((cols[:, 3], cols[:, 2], cols[:, 1], cols[:, 0])) if c["pattern"] == "popular_last" else np.arange(c["n"])
        idx = index_image(w, h, c["n"], c["pattern"], rng)
        if c["n"] <= w * h:  # every colour present
            flat = idx.reshape(-1)
            flat[rng.permutation(w * h)[:c["n"]]] = np.arange(c["n"])
        img = cols[order][idx]
        return np.ascontiguousarray(img[:, :, :BPP[ct]] if ct == 2 else img).reshape(-1)
    if gen == "grays":            # gray RGB / opaque gray RGBA: becomes a palette of <= 256 grays
        g = rng.randint(0, c["n"], (h, w)).astype(np.uint8)
        img = np.stack([g, g, g] + ([np.full_like(g, 255)] if ct == 3 else []), axis=2)
        return img.reshape(-1)
    if gen == "opaque":           # > 256 colours, alpha 255: RGBA -> RGB
        img = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
        img[:, :, 3] = 255
        return img.reshape(-1)
    if gen == "gray_alpha":       # gray RGBA, > 256 (gray, alpha) pairs, alpha 0 pixels: -> GrayAlpha
        g = rng.randint(0, 256, (h, w)).astype(np.uint8)
        a = rng.randint(0, 256, (h, w)).astype(np.uint8)
        a[rng.rand(h, w) < 0.2] = 0
        return np.stack([g, g, g, a], axis=2).reshape(-1)
    if gen == "keep":             # > 256 colours, alpha 0 pixels that carry colour: RGBA kept, optimize_alpha acts
        img = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
        img[:, :, 3][rng.rand(h, w) < 0.25] = 0
        return img.reshape(-1)
    if gen == "ga":               # GrayAlpha input with alpha 0 pixels
        img = rng.randint(0, 256, (h, w, 2)).astype(np.uint8)
        img[:, :, 1][rng.rand(h, w) < 0.3] = 0
        return img.reshape(-1)
    if gen == "gray":             # Gray input, small values: stays 8 bit (mod.rs:691-700)
        return rng.randint(0, 4, (h, w)).astype(np.uint8).reshape(-1)
    if gen == "rgb_noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8).reshape(-1)
    raise ValueError(c)


def cases(huge=False):
    cs = []

    def add(gen, w, h, ct, preset, expect, seed=1, **kw):
        tag = "_".join("%s%s" % (k[0], v) for k, v in sorted(kw.items()))
        cs.append(dict(gen=gen, w=w, h=h, color_type=ct, preset=preset, seed=seed, expect=expect,
                       name="%s%s_%dx%d_c%d_p%d_s%d" % (gen, "_" + tag if tag else "", w, h, ct, preset, seed), **kw))

    def pal(n, w, h, ct=3, alpha="opaque", pattern="noise", preset=1, seed=1):
        bits = 1 if n <= 2 else 2 if n <= 4 else 4 if n <= 16 else 8
        trns = ct == 3 and alpha != "opaque"
        add("pal", w, h, ct, preset, dict(ctype=3, depth=bits, plte=n, trns=trns), seed, n=n, alpha=alpha, pattern=pattern)

    for n in (1, 2, 3, 4, 5, 16, 17, 200, 256):
        pal(n, 80, 70, 3, "opaque", "noise", seed=n)
        pal(n, 96, 40, 2, "opaque", "smooth", seed=n + 1)
        pal(n, 71, 67, 3, "some", "popular", seed=n + 2)
        pal(n, 90, 75, 3, "zero", "smooth" if n % 2 else "noise", seed=n + 3)
    for n in (5, 16, 40, 200):
        pal(n, 120, 90, 3, "opaque", "popular_last", seed=n + 4)
        pal(n, 64, 100, 2, "opaque", "popular", seed=n + 5)
    # 257 colours: no palette; what remains is the colour-type reduction
    add("pal", 80, 70, 3, 1, dict(ctype=2, depth=8, plte=0, trns=False), 9, n=257, alpha="opaque", pattern="noise")
    add("pal", 80, 70, 3, 1, dict(ctype=6, depth=8, plte=0, trns=False), 10, n=257, alpha="some", pattern="noise")
    add("pal", 80, 70, 2, 1, dict(ctype=2, depth=8, plte=0, trns=False), 11, n=257, alpha="opaque", pattern="noise")
    # packed rows whose width is not a whole number of bytes, width 1 included
    for w in (1, 7, 9, 13, 130):
        pal(2, w, 50, 3, "opaque", "noise", seed=20 + w)
    for w in (1, 3, 5, 131):
        pal(4, w, 45, 2, "opaque", "noise", seed=30 + w)
    for w in (1, 3, 133):
        pal(13, w, 60, 3, "some", "noise", seed=40 + w)
    # the small-image rule counts pixels, not row bytes (filter.rs:77)
    for (w, h) in ((128, 64), (64, 64), (65, 64)):
        pal(2, w, h, 3, "opaque", "noise", seed=50 + w)
    # heights around the 32-row rule, presets 0 and 2
    for h in (8, 32, 33):
        pal(6, 300, h, 3, "opaque", "noise", seed=60 + h)
    pal(6, 300, 33, 3, "opaque", "noise", preset=2, seed=70)
    pal(3, 100, 70, 3, "zero", "popular", preset=2, seed=71)
    pal(200, 100, 70, 2, "opaque", "noise", preset=2, seed=72)
    add("pal", 100, 70, 3, 0, dict(ctype=6, depth=8, plte=0, trns=False), 73, n=6, alpha="opaque", pattern="noise")  # preset 0: nothing
    add("pal", 100, 24, 2, 0, dict(ctype=2, depth=8, plte=0, trns=False), 74, n=6, alpha="opaque", pattern="noise")
    # gray RGB / opaque gray RGBA: a palette of grays, never Gray
    add("grays", 120, 80, 2, 1, dict(ctype=3, depth=8, plte=256, trns=False), 80, n=256)
    add("grays", 120, 80, 3, 1, dict(ctype=3, depth=4, plte=16, trns=False), 81, n=16)
    # colour-type reductions
    add("opaque", 150, 100, 3, 1, dict(ctype=2, depth=8, plte=0, trns=False), 90)
    add("opaque", 67, 20, 3, 2, dict(ctype=2, depth=8, plte=0, trns=False), 91)
    add("gray_alpha", 150, 100, 3, 1, dict(ctype=4, depth=8, plte=0, trns=False), 92)
    add("gray_alpha", 75, 31, 3, 2, dict(ctype=4, depth=8, plte=0, trns=False), 93)
    add("keep", 150, 100, 3, 1, dict(ctype=6, depth=8, plte=0, trns=False), 94)
    add("keep", 40, 40, 3, 1, dict(ctype=6, depth=8, plte=0, trns=False), 95)
    add("keep", 75, 60, 3, 2, dict(ctype=6, depth=8, plte=0, trns=False), 96)
    add("ga", 200, 100, 1, 1, dict(ctype=4, depth=8, plte=0, trns=False), 97)
    add("ga", 200, 100, 1, 0, dict(ctype=4, depth=8, plte=0, trns=False), 98)
    add("gray", 200, 100, 0, 1, dict(ctype=0, depth=8, plte=0, trns=False), 99)
    add("rgb_noise", 150, 100, 2, 1, dict(ctype=2, depth=8, plte=0, trns=False), 100)
    # large
    add("pal", 1920, 1080, 3, 1, dict(ctype=3, depth=8, plte=200, trns=True), 110, n=200, alpha="some", pattern="popular")
    if huge:
        add("pal", 4096, 4096, 3, 1, dict(ctype=3, depth=4, plte=16, trns=False), 111, n=16, alpha="opaque", pattern="popular")
    return cs


def parse_png(png):
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    i, idat, ihdr, plte, trns = 8, [], None, b"", None
    while i < len(png):
        n, typ = struct.unpack(">I4s", png[i:i + 8])
        body = png[i + 8:i + 8 + n]
        if typ == b"IHDR": ihdr = struct.unpack(">IIBBBBB", body)
        if typ == b"PLTE": plte = body
        if typ == b"tRNS": trns = body
        if typ == b"IDAT": idat.append(body)
        i += 12 + n
    z = b"".join(idat)
    return ihdr, plte, trns, zlib.decompress(z), struct.unpack(">I", z[-4:])[0]


def main():
    import png_reduce_model as M
    huge = "--huge" in sys.argv
    cs = cases(huge)
    assert len({c["name"] for c in cs}) == len(cs)
    os.makedirs(os.path.join(HERE, "png_reduce"), exist_ok=True)
    branches = set()
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
        out = []
        for k, (c, line) in enumerate(zip(cs, res)):
            r = json.loads(line)
            assert r["ok"], (c, r)
            png = open(man["cases"][k]["output"], "rb").read()
            (w, h, depth, ctype, _, _, _), plte, trns, flt, trailer = parse_png(png)
            e = c["expect"]
            got = dict(ctype=ctype, depth=depth, plte=len(plte) // 3, trns=trns is not None)
            assert (w, h) == (c["w"], c["h"]) and got == e, ("the reference took another branch", c["name"], got, e)
            row = len(flt) // h
            assert row * h == len(flt) and trailer == zlib.adler32(flt)
            if trns is not None:
                assert len(trns) == len(plte) // 3  # all n alphas, no trimming
            info = {}
            M.reduce(make_input(c), w, h, c["color_type"], M.Opts.preset(c["preset"], M.NO_RAYON), info)
            branches.add(info.get("popular"))
            rec = dict(c, png_len=len(png), row_bytes=row - 1, plte_hex=plte.hex(), trns_hex=None if trns is None else trns.hex(),
                       filtered_len=len(flt), filtered_sha256=hashlib.sha256(flt).hexdigest(), adler32=trailer,
                       filters="".join(str(flt[y * row]) for y in range(h)), popular=info.get("popular"))
            if len(flt) <= STORE_LIMIT:
                open(os.path.join(HERE, "png_reduce", c["name"] + ".flt"), "wb").write(flt)
                rec["stored"] = True
            out.append(rec)
            print(c["name"], got, len(flt), "%08x" % trailer, info.get("popular"))
    assert {"skip", "front", "back"} <= branches, branches  # apply_most_popular_first: its skip and both halves
    dst = os.path.join(HERE, "png_reduce_cases.json")
    if not huge and os.path.exists(dst):  # keep a previously generated huge case
        out += [c for c in json.load(open(dst))["cases"] if c["w"] * c["h"] > 4000 * 4000]
    json.dump({"wasm_sha256": hashlib.sha256(open(os.path.join(ROOT, "oracle", "_ref", "pixo_bg.wasm"), "rb").read()).hexdigest(),
               "cases": out}, open(dst, "w"), indent=0)


if __name__ == "__main__":
    main()
