"""Writes tests/golden/jpeg_decode/ and tests/golden/jpeg_decode_cases.json: baseline JPEG files written by Pillow
(libjpeg-turbo) from synthetic content with a saturated flat patch, each with the pixels Pillow itself decodes from it
(zlib-compressed raw bytes) — the expectation is committed so that no test depends on which libjpeg a machine's Pillow
carries.  Run from the repository root with the library built (the tile case is sized from its tile):
    python tests/golden/make_golden_jpeg_decode.py"""
import hashlib
import io
import json
import os
import sys
import zlib

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
OUT = os.path.join(HERE, "jpeg_decode")
MODES = {"gray": None, "444": 0, "422": 1, "420": 2}  # Pillow's subsampling argument
MCU = {"gray": (8, 8), "444": (8, 8), "422": (16, 8), "420": (16, 16)}


def content(w, h, seed, noise):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + yy / 11.0), 128 + 90 * np.cos(xx / 5.0 - yy / 9.0), (xx * 5 + yy * 3) % 256], -1).astype(np.float64)
    base += rng.normal(0, noise, base.shape)
    base[h // 3:max(h // 2, h // 3 + 1), w // 4:max(w // 2, w // 4 + 1)] = [255, 0, 10]  # saturated: the clamps fire
    base[:max(h // 5, 1), (3 * w) // 4:] = [0, 0, 0]
    return np.clip(base, 0, 255).astype(np.uint8)


def write(w, h, mode, quality, seed, noise=12.0, **kw):
    im = Image.fromarray(content(w, h, seed, noise))
    if mode == "gray":
        im = im.convert("L")
    else:
        kw["subsampling"] = MODES[mode]
    b = io.BytesIO()
    im.save(b, "JPEG", quality=quality, **kw)
    return b.getvalue()


def segments(d):
    """[(marker, start, end)] of the segments in front of the scan; end of the last = start of the entropy-coded data"""
    out, p = [], 2
    while True:
        assert d[p] == 0xFF
        m, n = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        out.append((m, p, p + 2 + n))
        p += 2 + n
        if m == 0xDA:
            return out


def dqt16(d):
    """Every 8-bit DQT table rewritten with 16-bit entries"""
    out = bytearray(d[:2])
    for m, a, b in segments(d):
        seg = d[a:b]
        if m == 0xDB:
            body, o = bytearray(), 4
            while o < len(seg):
                assert seg[o] >> 4 == 0
                body += bytes([0x10 | seg[o]]) + b"".join(bytes([0, v]) for v in seg[o + 1:o + 65])
                o += 65
            seg = b"\xff\xdb" + (len(body) + 2).to_bytes(2, "big") + bytes(body)
        out += seg
    return bytes(out) + d[segments(d)[-1][2]:]


def odd_places(d):
    """Fill bytes in front of markers, a COM behind SOI, an APP5 and a COM between the tables and the scan"""
    out = bytearray(d[:2]) + b"\xff\xfe\x00\x07hello"
    for i, (m, a, b) in enumerate(segments(d)):
        if m == 0xDA:
            out += b"\xff\xff\xe5\x00\x06\xff\xd9\x00\xff" + b"\xff\xfe\x00\x02"
        out += b"\xff" * (i % 3) + d[a:b]
    return bytes(out) + d[segments(d)[-1][2]:]


def main():
    assert features.check_feature("libjpeg_turbo"), "the goldens are libjpeg-turbo's pixels"
    from pixo_amd import decode
    tx, ty = decode.decode_jpeg_tile_mcus()
    os.makedirs(OUT, exist_ok=True)
    cases, seed = [], 100

    def add(name, data, mode, **extra):
        px = np.asarray(Image.open(io.BytesIO(data)))
        assert px.dtype == np.uint8 and (px.ndim == 2) == (mode == "gray")
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        with open(os.path.join(OUT, name + ".px.z"), "wb") as f:
            f.write(zlib.compress(px.tobytes(), 9))
        cases.append(dict(name=name, mode=mode, w=px.shape[1], h=px.shape[0], color_type=0 if mode == "gray" else 2,
                          sha256=hashlib.sha256(px.tobytes()).hexdigest(), **extra))

    for mode in MODES:
        tile = (tx * MCU[mode][0] * 2 + 1, ty * MCU[mode][1] * 2 + 1)
        for (w, h) in [(1, 1), (2, 2), (3, 9), (4, 20), (5, 3), (7, 5), (8, 8), (9, 9), (16, 16), (17, 17), (33, 17), (50, 37), tile]:
            seed += 1
            big = (w, h) == tile
            add("%s_%dx%d_q80" % (mode, w, h), write(w, h, mode, 60 if big else 80, seed, noise=3.0 if big else 12.0), mode, tile=big)
        for q in (30, 95, 100):
            seed += 1
            add("%s_50x37_q%d" % (mode, q), write(50, 37, mode, q, seed), mode)
        seed += 1
        add("%s_33x17_q80_opt" % mode, write(33, 17, mode, 80, seed, noise=40.0, optimize=True), mode)
        mcus_row = -(-50 // MCU[mode][0])
        for blocks in (1, mcus_row, 5):
            seed += 1
            add("%s_50x37_q80_rst%d" % (mode, blocks), write(50, 37, mode, 80, seed, restart_marker_blocks=blocks), mode, restart=blocks)
    plain = write(50, 37, "420", 80, 900)
    add("420_50x37_q80_dqt16", dqt16(plain), "420")
    add("420_50x37_q80_odd_places", odd_places(write(50, 37, "420", 80, 901, restart_marker_blocks=3)), "420")
    add("gray_50x37_q80_odd_places", odd_places(write(50, 37, "gray", 80, 902)), "gray")
    with open(os.path.join(HERE, "jpeg_decode_cases.json"), "w") as f:
        json.dump(dict(tile_mcus=[tx, ty], cases=cases), f, indent=1)
    total = sum(os.path.getsize(os.path.join(OUT, n)) for n in os.listdir(OUT))
    print("%d cases, %d bytes under %s, largest %d" % (len(cases), total, OUT, max(os.path.getsize(os.path.join(OUT, n)) for n in os.listdir(OUT))))


if __name__ == "__main__":
    main()
