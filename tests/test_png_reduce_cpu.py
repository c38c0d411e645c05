"""CPU-only checks of the PNG prepare path: the C ABI's new symbols and structs, presets and builder, validation order and
messages, the host part of the palette case (pixo_hip_png_palette_order) against the PLTE order of every palette vector the
reference's wasm build made, and the kernels' arithmetic (png_reduce_math.h compiled for the host) against the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu_png_reduce_lib as E
import png_reduce_cases as PC
import png_reduce_model as M
from pixo_amd import ColorType, _lib, error, png

NEW = ["pixo_hip_png_options_from_preset", "pixo_hip_png_prepare", "pixo_hip_png_prepare_device", "pixo_hip_png_palette_order"]


def test_new_symbols_are_declared_listed_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pixo_hip.h")).read()
    declared = set(re.findall(r"\b(pixo_(?:hip|jpeg)_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert declared == set(_lib.SYMBOLS)


def test_struct_layouts_match_header():
    assert C.sizeof(_lib.PngOptionsC) == 20 and _lib.PngOptionsC.flags.offset == 16
    assert C.sizeof(_lib.PngLayoutC) == 12 + 1024 and _lib.PngLayoutC.palette.offset == 12


def test_presets_follow_reference():
    # mod.rs:129-198
    L = _lib.load()
    want = {0: (png.FilterStrategy.ADAPTIVE_FAST, 0, 0, 0, 2, 0, 0), 1: (png.FilterStrategy.ADAPTIVE, 1, 1, 1, 6, 0, 1),
            2: (png.FilterStrategy.BIGRAMS, 1, 1, 1, 9, 1, 1)}
    for preset in (0, 1, 2, 3, 77):
        o = _lib.PngOptionsC()
        L.pixo_hip_png_options_from_preset(C.byref(o), 7, 9, preset)
        got = (o.filter_strategy, o.optimize_alpha, o.reduce_color_type, o.reduce_palette, o.compression_level, o.optimal_compression, o.strip_metadata)
        assert (o.width, o.height, o.color_type, o.flags) == (7, 9, 3, 0)
        assert got == want.get(preset, want[1])
        p = png.PngOptions.from_preset(7, 9, preset).to_c()
        assert bytes(p) == bytes(o)


def test_builder_follows_reference():
    # mod.rs:220-340: defaults are preset 0's; .preset() keeps dimensions and colour type; later setters override
    d = png.PngOptions.builder(3, 4).build()
    assert (d.color_type, d.filter_strategy, d.compression_level) == (ColorType.Rgba, png.FilterStrategy.ADAPTIVE_FAST, 2)
    assert not (d.optimize_alpha or d.reduce_color_type or d.reduce_palette or d.strip_metadata or d.optimal_compression)
    o = png.PngOptions.builder(10, 20).color_type(ColorType.Rgb).preset(2).reduce_palette(False).filter_strategy(png.FilterStrategy.PAETH).build()
    assert (o.width, o.height, o.color_type) == (10, 20, ColorType.Rgb)
    assert o.optimize_alpha and o.reduce_color_type and not o.reduce_palette and o.optimal_compression
    assert o.filter_strategy == png.FilterStrategy.PAETH and o.compression_level == 9
    assert o.full_size() == 20 * (10 * 3 + 1)
    assert not hasattr(png.PngOptionsBuilder, "lossy") and not hasattr(png.PngOptionsBuilder, "quantization")


def test_validation_order_and_messages():
    px = np.zeros(64, np.uint8)
    B = png.PngOptions.builder
    with pytest.raises(error.InvalidDimensions, match="Invalid image dimensions: 0x4"):
        png.prepare(px, B(0, 4).build())
    with pytest.raises(error.InvalidDimensions, match="Invalid image dimensions: 16777217x0"):
        png.prepare(px, B(16777217, 0).build())  # dimensions before size
    with pytest.raises(error.ImageTooLarge, match="Image 16777217x1 exceeds maximum dimension 16777216"):
        png.prepare(px, B(16777217, 1).build())  # size before length
    with pytest.raises(error.InvalidDataLength, match="Invalid pixel data length: expected 64 bytes, got 63"):
        png.prepare(px[:63], B(4, 4).build())
    with pytest.raises(error.InvalidDataLength, match="Invalid pixel data length: expected 48 bytes, got 64"):
        png.prepare(px, B(4, 4).color_type(ColorType.Rgb).build())
    L = _lib.load()
    o, lay, n, ad = B(4, 4).build().to_c(), _lib.PngLayoutC(), C.c_size_t(), C.c_uint32()
    assert L.pixo_hip_png_prepare(px.ctypes.data, 64, None, None, 0, C.byref(n), C.byref(lay), C.byref(ad)) == -6
    assert L.pixo_hip_png_prepare(None, 64, C.byref(o), None, 0, C.byref(n), C.byref(lay), C.byref(ad)) == -6
    assert L.pixo_hip_png_prepare_device(None, C.byref(o), None, C.byref(lay), C.byref(n), C.byref(ad)) == -6
    assert L.pixo_hip_png_palette_order(None, None, 3, None) == -6


PALETTES = [c for c in PC.small() if c["expect"]["ctype"] == 3]


@pytest.mark.parametrize("c", PALETTES, ids=[c["name"] for c in PALETTES])
def test_palette_order_equals_reference_plte(c):
    """Histogram and matrix by the model, the order by the library's host code: the palette in that order is the PLTE (+ tRNS)
    the reference wrote."""
    px = PC.make_input(c).reshape(c["h"], c["w"], -1).astype(np.uint32)
    keys = (px[:, :, 0] << 24) | (px[:, :, 1] << 16) | (px[:, :, 2] << 8) | (px[:, :, 3] if px.shape[2] == 4 else 255)
    uniq = np.unique(keys)
    counts, matrix = M.statistics(np.searchsorted(uniq, keys).astype(np.uint8), len(uniq))
    order = png.palette_order(counts, matrix)
    assert sorted(order) == list(range(len(uniq)))
    pal = uniq[order.astype(np.int64)]
    assert b"".join(bytes([int(k) >> 24, (int(k) >> 16) & 255, (int(k) >> 8) & 255]) for k in pal).hex() == c["plte_hex"]
    if c["trns_hex"] is not None:
        assert bytes(int(k) & 255 for k in pal).hex() == c["trns_hex"]
    assert list(order) == M.palette_order(counts, matrix)
    m2 = matrix.copy()
    np.fill_diagonal(m2, 12345)  # nothing reads the diagonal
    assert np.array_equal(png.palette_order(counts, m2), order)


def test_palette_order_counters_wrap_like_the_release_build():
    counts = np.array([5, 5, 5, 5], np.uint32)
    m = np.zeros((4, 4), np.uint32)
    m[0, 1] = m[1, 0] = 0xFFFFFFF0
    m[2, 0] = m[0, 2] = 0x20
    m[2, 1] = m[1, 2] = 0xFFFFFFF0  # 0x20 + 0xFFFFFFF0 wraps to 0x10
    m[3, 0] = m[0, 3] = 0x11
    assert list(png.palette_order(counts, m)) == M.palette_order(counts, m)


def test_ihdr_plte_trns_chunks():
    import struct, zlib
    lay = png.PngLayout(_lib.PngLayoutC(3, 2, 1, 1, 5, 3, ((C.c_uint8 * 4) * 256)((1, 2, 3, 255), (4, 5, 6, 0), (7, 8, 9, 255))))
    b = png.ihdr_plte_trns(lay, 20, 10)
    assert b[:8] == struct.pack(">I", 13) + b"IHDR" and b[8:21] == struct.pack(">IIBBBBB", 20, 10, 2, 3, 0, 0, 0)
    assert struct.unpack(">I", b[21:25])[0] == zlib.crc32(b[4:21])
    assert b[25:33] == struct.pack(">I", 9) + b"PLTE" and b[33:42] == bytes(range(1, 10))
    assert b[46:54] == struct.pack(">I", 3) + b"tRNS" and b[54:57] == b"\xff\x00\xff" and len(b) == 61


@pytest.mark.parametrize("seed", range(120))
def test_kernel_arithmetic_on_the_host_equals_model(seed):
    """png_reduce_math.h compiled for the host (key lookup, reduced_byte for every form) gives the model's reduced rows."""
    px, w, h, ct, sw, strategy, flags = PC.random_case(seed)
    o = M.Opts(strategy, sw["optimize_alpha"], sw["reduce_color_type"], sw["reduce_palette"], flags)
    res = M.reduce(px, w, h, ct, o)
    M.optimize_alpha(res, o)
    spp, rb = M.BPP[ct], res["rows"].shape[1]
    if res["palette"] is not None:
        keys = np.array(sorted((p[0] << 24) | (p[1] << 16) | (p[2] << 8) | p[3] for p in res["palette"]), np.uint32)
        idx = E.index(px, w * h, spp, keys)
        bmap = np.zeros(256, np.uint8)
        bmap[np.array(res["order"])] = np.arange(len(keys), dtype=np.uint8)
        assert E.lib().emu_png_palette_bits(len(keys)) == res["bit_depth"]
        got = E.convert(idx, E.FORM_INDEX, 1, res["bit_depth"], 0, w, h, rb, bmap)
    elif res["color_type_byte"] == 0 and ct in (2, 3):
        assert E.lib().emu_png_gray_bits(int(px.reshape(-1, spp)[:, 0].max())) == res["bit_depth"]
        got = E.convert(px, E.FORM_GRAY, spp, res["bit_depth"], 0, w, h, rb)
    elif res["color_type_byte"] == 2 and ct == 3:
        got = E.convert(px, E.FORM_RGB, 4, 8, 0, w, h, rb)
    elif res["color_type_byte"] == 4 and ct == 3:
        got = E.convert(px, E.FORM_GA, 4, 8, o.optimize_alpha, w, h, rb)
    elif o.optimize_alpha and ct in (1, 3):
        got = E.convert(px, E.FORM_ZERO_ALPHA, spp, 8, 1, w, h, rb)
    else:
        got = px.reshape(h, rb)
    assert np.array_equal(got, res["rows"])
