"""CPU-only checks of the PNG lossy mode: the C ABI's new symbols and struct, options, presets and builder against the
reference (src/png/mod.rs:203-213, :292-325), validation order and messages, the host part (pixo_hip_png_median_cut) against
the model on every vector's histogram and on adversarial ones, and the kernels' arithmetic (png_quantize_math.h compiled for
the host) against the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu_png_quantize_lib as E
import png_quantize_cases as QC
import png_quantize_model as M
from pixo_amd import ColorType, _lib, error, png

NEW = ["pixo_hip_png_quantize", "pixo_hip_png_quantize_device", "pixo_hip_png_encode_lossy", "pixo_hip_png_encode_lossy_device",
       "pixo_hip_png_median_cut", "pixo_hip_debug_png_dither_stats"]


def test_new_symbols_are_declared_listed_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pixo_hip.h")).read()
    declared = set(re.findall(r"\b(pixo_(?:hip|jpeg)_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert declared == set(_lib.SYMBOLS)
    assert re.search(r"PIXO_PNG_QUANT_OFF = 0, PIXO_PNG_QUANT_AUTO = 1, PIXO_PNG_QUANT_FORCE = 2", hdr)


def test_struct_layouts():
    assert C.sizeof(_lib.PngQuantizationC) == 4 and _lib.PngQuantizationC.max_colors.offset == 2
    assert C.sizeof(_lib.PngOptionsC) == 20 and C.sizeof(_lib.PngLayoutC) == 12 + 1024  # quantisation travels beside them


def test_options_presets_and_builder_follow_reference():
    Q, Mode = png.QuantizationOptions, png.QuantizationMode
    assert (int(Mode.OFF), int(Mode.AUTO), int(Mode.FORCE)) == (0, 1, 2)
    d = Q()
    assert (d.mode, d.max_colors, d.dithering) == (Mode.OFF, 256, False)
    for preset in (0, 1, 2):
        assert png.PngOptions.from_preset(3, 4, preset).quantization == Q()
        assert png.PngOptions.from_preset_with_lossless(3, 4, preset, True).quantization == Q()
        o = png.PngOptions.from_preset_with_lossless(3, 4, preset, False)  # mod.rs:203-213
        assert o.quantization == Q(Mode.AUTO, 256, True)
        assert bytes(o.to_c()) == bytes(png.PngOptions.from_preset(3, 4, preset).to_c())
    b = png.PngOptions.builder(5, 6).quantization_mode(Mode.FORCE).quantization_max_colors(17).quantization_dithering(True).build()
    assert b.quantization == Q(Mode.FORCE, 17, True) and bytes(b.quantization.to_c()) == bytes([2, 1, 17, 0])
    assert png.PngOptions.builder(5, 6).quantization_mode(1).build().quantization == Q(Mode.AUTO, 256, False)  # the mode alone (:297-300)
    # .preset() replaces the options but for dimensions and colour type (:327-334): quantisation goes back to its default
    assert png.PngOptions.builder(5, 6).quantization_mode(2).preset(1).build().quantization == Q()
    assert png.PngOptions.builder(5, 6).build().quantization is not png.PngOptions.builder(5, 6).build().quantization
    assert not hasattr(png.PngOptionsBuilder, "lossy") and not hasattr(png.PngOptionsBuilder, "quantization")


def test_validation_order_and_messages():
    px = np.zeros(64, np.uint8)

    def opts(w, h, ct=ColorType.Rgba):
        return png.PngOptions.builder(w, h).color_type(ct).quantization_mode(png.QuantizationMode.FORCE).build()

    for call in (png.quantize, png.encode):
        with pytest.raises(error.InvalidDimensions, match="Invalid image dimensions: 0x4"):
            call(px, opts(0, 4))
        with pytest.raises(error.InvalidDimensions, match="Invalid image dimensions: 16777217x0"):
            call(px, opts(16777217, 0))
        with pytest.raises(error.ImageTooLarge, match="Image 16777217x1 exceeds maximum dimension 16777216"):
            call(px, opts(16777217, 1))
        with pytest.raises(error.InvalidDataLength, match="Invalid pixel data length: expected 64 bytes, got 63"):
            call(px[:63], opts(4, 4))
        with pytest.raises(error.InvalidDataLength, match="Invalid pixel data length: expected 48 bytes, got 64"):
            call(px, opts(4, 4, ColorType.Rgb))
    L = _lib.load()
    o, q = opts(4, 4).to_c(), png.QuantizationOptions(2).to_c()
    p, n, a = C.POINTER(C.c_uint8)(), C.c_size_t(), C.c_uint8()
    pal, pn, tn = np.zeros((256, 4), np.uint8), C.c_uint32(), C.c_uint32()
    out = np.zeros(16, np.uint8)

    def message():
        return L.pixo_hip_last_error().decode()

    # the checks of pixo_hip_png_prepare first, in its order, then the quantization struct
    bad = opts(0, 4).to_c()
    assert L.pixo_hip_png_encode_lossy(px.ctypes.data, 64, C.byref(bad), None, C.byref(p), C.byref(n)) == -1 and "Invalid image dimensions" in message()
    assert L.pixo_hip_png_encode_lossy(px.ctypes.data, 63, C.byref(o), None, C.byref(p), C.byref(n)) == -2 and "Invalid pixel data length" in message()
    assert L.pixo_hip_png_encode_lossy(px.ctypes.data, 64, C.byref(o), None, C.byref(p), C.byref(n)) == -6 and "null argument 'quantization'" in message()
    assert L.pixo_hip_png_encode_lossy(None, 64, C.byref(o), None, C.byref(p), C.byref(n)) == -6 and "null argument 'data'" in message()
    assert L.pixo_hip_png_encode_lossy(px.ctypes.data, 64, None, C.byref(q), C.byref(p), C.byref(n)) == -6
    assert L.pixo_hip_png_encode_lossy_device(None, C.byref(o), C.byref(q), C.byref(p), C.byref(n)) == -6
    assert L.pixo_hip_png_quantize(px.ctypes.data, 64, C.byref(o), None, out.ctypes.data, 16, pal.ctypes.data, C.byref(pn), C.byref(tn), C.byref(a)) == -6
    assert "null argument 'quantization'" in message()
    assert L.pixo_hip_png_quantize_device(None, C.byref(o), C.byref(q), None, pal.ctypes.data, C.byref(pn), C.byref(tn), C.byref(a)) == -6
    q.mode = 3
    assert L.pixo_hip_png_encode_lossy(px.ctypes.data, 64, C.byref(o), C.byref(q), C.byref(p), C.byref(n)) == -6 and "unknown PNG quantization mode" in message()
    assert L.pixo_hip_png_median_cut(None, None, 3, 4, None, None) == -6
    k = np.zeros(3, np.uint32)
    assert L.pixo_hip_png_median_cut(k.ctypes.data, k.ctypes.data, 0, 4, pal.ctypes.data, C.byref(pn)) == -6
    assert L.pixo_hip_png_median_cut(k.ctypes.data, k.ctypes.data, 8193, 4, pal.ctypes.data, C.byref(pn)) == -6


# ---- median cut ------------------------------------------------------------------------------------------------------------

def check_median_cut(colors, counts, max_colors):
    got = QC.palette_keys(png.median_cut(colors, counts, max_colors))
    assert got == M.median_cut(np.asarray(colors, np.uint32), np.asarray(counts, np.uint32), min(max_colors, 256))
    return got


@pytest.mark.parametrize("c", QC.APPLIED, ids=[c["name"] for c in QC.APPLIED])
def test_median_cut_on_every_vectors_histogram(c):
    colors, counts = M.histogram(M.keys_of(QC.make_input(c), QC.BPP[c["color_type"]]))
    assert check_median_cut(colors, counts, 256) == QC.model(c)[2]["cut"]


@pytest.mark.parametrize("max_colors", [0, 1, 2, 255, 300])
@pytest.mark.parametrize("kind", ["equal_counts", "two_colours", "score_ties", "random", "one_colour"])
def test_median_cut_adversarial(kind, max_colors):
    rng = np.random.RandomState(len(kind) * 1000 + max_colors)
    if kind == "equal_counts":
        colors, counts = np.unique(rng.randint(0, 1 << 32, 700, dtype=np.uint64).astype(np.uint32)), None
        counts = np.full(len(colors), 7, np.uint32)
    elif kind == "two_colours":
        colors, counts = np.array([0x10203040, 0xF0E0D0C0], np.uint32), np.array([1, 1000000], np.uint32)
    elif kind == "score_ties":  # ranges 60 / 30 / 120 / 40: the scores 2 R = 4 G = 1 B = 3 A = 120 tie, in every box again and again
        r, g, b, a = np.meshgrid(np.arange(0, 61, 20), np.arange(0, 31, 10), np.arange(0, 121, 40), np.arange(0, 41, 10), indexing="ij")
        colors = ((r << 24) | (g << 16) | (b << 8) | a).reshape(-1).astype(np.uint32)
        counts = (1 + np.arange(len(colors)) % 3).astype(np.uint32)
    elif kind == "one_colour":
        colors, counts = np.array([0x01020304], np.uint32), np.array([9], np.uint32)
    else:
        colors = np.unique(rng.randint(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32))
        counts = rng.randint(1, 50000, len(colors)).astype(np.uint32)
        order = rng.permutation(len(colors))  # not in key order: as after the 8,192 cut
        colors, counts = colors[order], counts[order]
    got = check_median_cut(colors, counts, max_colors)
    assert 1 <= len(got) <= max(min(max_colors, 256), 1)


# ---- png_quantize_math.h on the host ---------------------------------------------------------------------------------------

def test_distance_cell_expansion_and_search_equal_model():
    rng = np.random.RandomState(5)
    L = E.lib()
    edge = [0x00000000, 0xFFFFFFFF, 0xFF0000FF, 0x00FF0000, 0x0000FF00, 0x000000FF, 0x80808080]
    cols = edge + [int(v) for v in rng.randint(0, 1 << 32, 400, dtype=np.uint64)]
    for a in cols[:60]:
        want = M.distances(M.rgba(cols), M.rgba([a])[0])
        assert [L.emu_pngq_distance(c, a) for c in cols] == [int(v) for v in want]
    cells = np.arange(64 ** 3)
    want = (M.expand6(cells >> 12) << 24) | (M.expand6((cells >> 6) & 63) << 16) | (M.expand6(cells & 63) << 8) | 255
    assert [L.emu_pngq_cell_color(int(c)) for c in (0, 1, 63, 64, 4095, 4096, 262143, 12345, 77777)] == [int(want[c]) for c in (0, 1, 63, 64, 4095, 4096, 262143, 12345, 77777)]
    for n in (1, 2, 16, 256):
        pal = [int(v) for v in rng.randint(0, 1 << 32, n, dtype=np.uint64)]
        pal[n // 2] = pal[0]  # a duplicate: the first of two equal entries wins
        probe = cols[:80] + pal[:8]
        assert [E.nearest(pal, c) for c in probe] == [int(v) for v in M.nearest_all(M.rgba(probe), pal)]
    pal = [c | 255 for c in cols[:200]]
    assert np.array_equal(E.lut(pal), M.build_lut(pal))


def test_dither_step_equals_model():
    L = E.lib()
    for c in (0, 1, 7, 128, 254, 255):
        for e in list(range(-16 * 255, -16 * 255 + 40)) + list(range(-40, 40)) + list(range(16 * 255 - 40, 16 * 255 + 1)):
            t = 16 * c + e
            assert L.emu_pngq_dither_adjust(c, e) == (0 if t < 0 else min(t >> 4, 255))
    assert L.emu_pngq_dither_adjust(0, -1) == 0 and L.emu_pngq_dither_adjust(255, 1) == 255 and L.emu_pngq_dither_adjust(250, 16 * 255) == 255
    pal = [0x000000FF, 0xFFFFFFFF, 0x80402010, 0x10204080]
    table = M.build_lut(pal)
    idx, e = E.dither_pixel(table, pal, 0x0A141EFF, [-4000, 16 * 255, 5])  # t < 0 in red, t >> 4 > 255 in green
    assert (idx, e) == (int(table[((0 >> 2) << 12) | ((255 >> 2) << 6) | (30 >> 2)]), [0 - (pal[idx] >> 24), 255 - ((pal[idx] >> 16) & 255), 30 - ((pal[idx] >> 8) & 255)])
    idx, e = E.dither_pixel(table, pal, 0x80402011, [0, 0, 0])  # alpha 17: the search, not the table
    assert idx == 2 and e == [0, 0, 0]


@pytest.mark.parametrize("w,h,spp", [(1, 1, 3), (1, 70, 4), (2, 3, 3), (3, 2, 4), (70, 1, 3), (5, 200, 3), (67, 129, 4), (130, 65, 3)])
def test_dither_image_through_band_carries_equals_model(w, h, spp):
    c = QC.force_case(w, h, spp - 1, 300, w + h)
    keys = M.keys_of(QC.make_input(c), spp)
    pal = M.median_cut(*M.histogram(keys), 16)
    table = M.build_lut(pal)
    assert np.array_equal(E.dither_image(keys, w, h, table, pal), M.dither(M.rgba(keys), w, h, table, pal))
