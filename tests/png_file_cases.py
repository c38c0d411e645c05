"""The whole-file PNG vectors (tests/golden/png_files.json, made by the reference's own wasm build:
tests/golden/make_golden_png_files.py), their inputs, and the parsing a test needs.  Test harness only."""
import json
import os
import struct
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_png_files as MG  # noqa: E402  (input generators only; nothing is run)

CASES = json.load(open(os.path.join(HERE, "golden", "png_files.json")))["cases"]
make_input = MG.make_input
IDAT_BYTES = 256 * 1024


def stored_file(c):
    return open(os.path.join(HERE, "golden", "png_files", c["name"] + ".png"), "rb").read()


def parse(png):
    """-> (IDAT bodies, [(type, body)] of every other chunk in order); every chunk's CRC is checked"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    i, idat, other = 8, [], []
    while i < len(png):
        n, typ = struct.unpack(">I4s", png[i:i + 8])
        body = png[i + 8:i + 8 + n]
        assert len(body) == n
        assert struct.unpack(">I", png[i + 8 + n:i + 12 + n])[0] == zlib.crc32(typ + body), "CRC of chunk %r" % typ
        (idat.append(body) if typ == b"IDAT" else other.append((typ.decode(), body)))
        i += 12 + n
    assert i == len(png)
    return idat, other


def options(c):
    from pixo_amd import ColorType, png
    return png.PngOptions.builder(c["w"], c["h"]).color_type(ColorType(c["color_type"])).preset(c["preset"]).flags(png.NO_RAYON).build()
