"""The PNG lossy-mode vectors (tests/golden/png_quantize_cases.json, made by the reference's own wasm build:
tests/golden/make_golden_png_quantize.py), their inputs, the model's results for them (computed once, shared, never
changed) and the inputs of the options the wasm cannot reach.  Test harness only."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_png_quantize as MG  # noqa: E402  (input generators only; nothing is run)
import png_quantize_model as M  # noqa: E402

CASES = json.load(open(os.path.join(HERE, "golden", "png_quantize_cases.json")))["cases"]
APPLIED = [c for c in CASES if c["applied"]]
DECLINED = [c for c in CASES if not c["applied"]]
make_input = MG.make_input
BPP = MG.BPP
IDAT_BYTES = 256 * 1024


def stored_file(c):
    return open(os.path.join(HERE, "golden", "png_quantize", c["name"] + ".png"), "rb").read()


def options(c):
    """The wasm's options for a case: preset, Auto, 256 colours, dithering (mod.rs:203-213)"""
    from pixo_amd import ColorType, png
    o = png.PngOptions.from_preset_with_lossless(c["w"], c["h"], c["preset"], False)
    o.color_type, o.flags = ColorType(c["color_type"]), png.NO_RAYON
    return o


_MODEL = {}


def model(c, max_colors=256, dithering=True):
    """(palette keys, indices, stage record) of the model for a case's pixels"""
    k = (c["name"], max_colors, dithering)
    if k not in _MODEL:
        palette, idx, rec = M.quantize(make_input(c), c["w"], c["h"], BPP[c["color_type"]], max_colors, dithering)
        idx.setflags(write=False)
        _MODEL[k] = (palette, idx, rec)
    return _MODEL[k]


def force_case(w, h, ct, n, seed):
    """An input for the options only Force reaches: the golden generator's random palette over a smooth field"""
    return dict(gen="pal", w=w, h=h, color_type=ct, preset=1, seed=seed, n=n, name="force_n%d_%dx%d_c%d_s%d" % (n, w, h, ct, seed))


def palette_keys(palette_rgba):
    return [(int(p[0]) << 24) | (int(p[1]) << 16) | (int(p[2]) << 8) | int(p[3]) for p in palette_rgba]
