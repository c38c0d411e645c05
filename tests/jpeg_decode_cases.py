"""The JPEG decoder's cases: baseline files written by Pillow (tests/golden/make_golden_jpeg_decode.py) with the pixels
libjpeg-turbo decodes from them, both committed under tests/golden/jpeg_decode/ — no test depends on which libjpeg a
machine's Pillow carries.  Shapes 1x1 .. 50x37 — among them 2x2, 3x9 and 4x20, too narrow for libjpeg's fancy upsamplers, and
5x3, the narrowest that gets them — and one image of two tiles and a pixel each way, for gray, 4:4:4, 4:2:2 and 4:2:0; qualities 30 / 80 / 95 / 100; optimised tables; restart intervals; 16-bit DQT; fill bytes, APPn and COM in odd places.
Expectations and model results are computed once, shared and never changed.  Test harness only."""
import hashlib
import json
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "jpeg_decode")
with open(os.path.join(HERE, "golden", "jpeg_decode_cases.json")) as _f:
    _J = json.load(_f)
TILE_MCUS = tuple(_J["tile_mcus"])  # the tile the tile cases were sized for
CASES = _J["cases"]
IDS = [c["name"] for c in CASES]
# The files no encoder writes (tests/golden/make_golden_jpeg_decode_synth.py, written by tests/jpeg_write.py): table assignments,
# component ids, segment orders, long codes, ZRL and blocks without an end, restarts with fill bytes, odd file ends — 50x37 and
# 17x17.  Where an entry has "pillow", Pillow refuses the file and the committed pixels are the sequential model's.
SYNTH_DIR = os.path.join(HERE, "golden", "jpeg_decode_synth")
with open(os.path.join(HERE, "golden", "jpeg_decode_synth_cases.json")) as _f:
    SYNTH = json.load(_f)["cases"]
for _c in SYNTH:
    _c["dir"] = SYNTH_DIR
SYNTH_IDS = [c["name"] for c in SYNTH]
MCU = {"gray": (8, 8), "444": (8, 8), "422": (16, 8), "420": (16, 16)}
_data, _expected, _model = {}, {}, {}


def path(c):
    return os.path.join(c.get("dir", DIR), c["name"] + ".jpg")


def data(c) -> bytes:
    if c["name"] not in _data:
        with open(path(c), "rb") as f:
            _data[c["name"]] = f.read()
    return _data[c["name"]]


def expected(c) -> bytes:
    """Pillow's pixels of the file, as committed"""
    if c["name"] not in _expected:
        with open(os.path.join(c.get("dir", DIR), c["name"] + ".px.z"), "rb") as f:
            px = zlib.decompress(f.read())
        assert len(px) == c["w"] * c["h"] * (c["color_type"] + 1) and hashlib.sha256(px).hexdigest() == c["sha256"], c["name"]
        _expected[c["name"]] = px
    return _expected[c["name"]]


def model(c):
    """(frame, coefficients per component) of the sequential model, shared"""
    import jpeg_decode_model as M
    if c["name"] not in _model:
        _model[c["name"]] = M.coefficients(data(c))
    return _model[c["name"]]


def by_name(name):
    return next(c for c in CASES + SYNTH if c["name"] == name)


def small(limit=64 * 64):
    return [c for c in CASES if c["w"] * c["h"] <= limit]


def mismatch(got: bytes, c) -> str:
    """'' when `got` is the expectation, else where it first differs"""
    want = expected(c)
    if got == want:
        return ""
    if len(got) != len(want):
        return "%s: %d bytes, expected %d" % (c["name"], len(got), len(want))
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    bad = np.flatnonzero(a != b)
    bpp = c["color_type"] + 1
    p = int(bad[0]) // bpp
    return "%s: %d of %d bytes differ, first at pixel (%d, %d) channel %d: got %d, expected %d, max difference %d" % (
        c["name"], bad.size, a.size, p % c["w"], p // c["w"], int(bad[0]) % bpp, a[bad[0]], b[bad[0]], int(np.abs(a.astype(int) - b.astype(int)).max()))
