"""The vectors of the PNG reductions (tests/golden/png_reduce_cases.json, made by the reference's own wasm build:
tests/golden/make_golden_png_reduce.py) and what a result is compared with.  Also the seeded random cases the GPU suite
and the host emulation run against the model.  Test harness only."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_png_reduce as MG  # noqa: E402  (input generators only; nothing is run)

CASES = json.load(open(os.path.join(HERE, "golden", "png_reduce_cases.json")))["cases"]
PNG_CT = {0: 0, 1: 4, 2: 2, 3: 6}
make_input = MG.make_input


def small(limit=2100 * 1100):
    return [c for c in CASES if c["w"] * c["h"] <= limit]


def check(c, stream, layout, adler):
    """stream: uint8 array; layout: dict as png_reduce_model.prepare returns it"""
    e = c["expect"]
    assert (layout["color_type_byte"], layout["bit_depth"]) == (e["ctype"], e["depth"])
    assert layout["row_bytes"] == c["row_bytes"]
    plte = b"".join(bytes(p[:3]) for p in layout["palette"])
    assert plte.hex() == c["plte_hex"]
    trns = bytes(p[3] for p in layout["palette"]).hex() if layout["has_trns"] else None
    assert trns == c["trns_hex"]
    row = c["row_bytes"] + 1
    assert stream.size == c["filtered_len"]
    assert "".join(str(int(f)) for f in stream[::row]) == c["filters"]
    assert hashlib.sha256(stream.tobytes()).hexdigest() == c["filtered_sha256"]
    assert adler == c["adler32"]
    if c.get("stored"):
        assert stream.tobytes() == open(os.path.join(HERE, "golden", "png_reduce", c["name"] + ".flt"), "rb").read()


def random_case(seed):
    """-> (pixels, w, h, color_type, switches dict, strategy, flags): sizes 1x1 .. 700x500, all four colour types, every
    switch combination, colour counts straddling 2 / 4 / 16 / 256."""
    rng = np.random.RandomState(1000 + seed)
    ct = int(rng.randint(0, 4))
    if seed % 10 == 0:
        w, h = int(rng.randint(300, 701)), int(rng.randint(200, 501))
    elif seed % 10 == 1:
        w, h = [(1, 1), (1, 37), (53, 1), (2, 2), (700, 500), (64, 64), (65, 63)][(seed // 10) % 7]
    else:
        w, h = int(rng.randint(1, 160)), int(rng.randint(1, 120))
    sw = dict(optimize_alpha=bool(seed & 1), reduce_color_type=bool(seed & 2), reduce_palette=bool(seed & 4))
    strategy = int(rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 6, 7, 8]))
    flags = int(rng.randint(0, 2))
    spp = (1, 2, 3, 4)[ct]
    kind = int(rng.randint(0, 6))
    if kind <= 2:      # n colours, n around the bit-depth and palette limits
        n = int(rng.choice([1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 300]))
        cols = rng.randint(0, 256, (n, spp)).astype(np.uint8)
        if kind == 1:  # grays
            cols[:, :3 if spp >= 3 else 1] = cols[:, :1]
            if rng.rand() < 0.5 and spp >= 3:
                cols[:, 0:3] = (cols[:, :1] % [2, 4, 16][int(rng.randint(0, 3))])
        if spp in (2, 4):
            mode = int(rng.randint(0, 3))
            if mode == 0:
                cols[:, -1] = 255
            elif mode == 1:
                cols[::2, -1] = 0
        idx = rng.randint(0, n, (h, w)) if rng.rand() < 0.5 else ((np.arange(w)[None, :] // 3 + np.arange(h)[:, None] // 2) % n)
        img = cols[idx]
    else:
        img = rng.randint(0, 256, (h, w, spp)).astype(np.uint8)
        if kind == 3 and spp >= 3:
            img[:, :, 1] = img[:, :, 0]; img[:, :, 2] = img[:, :, 0]
        if spp in (2, 4):
            if kind == 4:
                img[:, :, -1] = 255
            elif rng.rand() < 0.6:
                img[:, :, -1][rng.rand(h, w) < 0.2] = 0
    return np.ascontiguousarray(img).reshape(-1), w, h, ct, sw, strategy, flags
