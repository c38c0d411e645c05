"""PNG lossy mode on the device against the vectors the reference's own wasm build made (tests/golden/png_quantize_cases.json)
and, for the options the wasm cannot reach, against the model that reproduces every one of those vectors
(tests/png_quantize_model.py, pinned by tests/test_png_quantize_model.py).  Everything but the IDAT body's own DEFLATE is
compared byte for byte; the IDAT body by what it inflates to."""
import hashlib
import struct
import zlib

import numpy as np
import pytest

import png_file_cases as PF
import png_quantize_cases as QC
import png_quantize_model as M

pytestmark = pytest.mark.gpu


def png():
    from pixo_amd import png as P
    return P


def check_file(c, out):
    idat, other = PF.parse(out)  # (checks every chunk's CRC)
    assert out[:8] == b"\x89PNG\r\n\x1a\n"
    assert [[t, b.hex()] for t, b in other] == c["chunks"], "a chunk around IDAT differs from the reference's"
    z = b"".join(idat)
    assert z[:2].hex() == c["zlib_header"] and struct.unpack(">I", z[-4:])[0] == c["adler32"]
    assert all(len(b) == QC.IDAT_BYTES for b in idat[:-1]) and 0 < len(idat[-1]) <= QC.IDAT_BYTES
    stream = zlib.decompress(z)
    assert len(stream) == c["stream_len"] and hashlib.sha256(stream).hexdigest() == c["stream_sha256"]


@pytest.mark.parametrize("c", QC.CASES, ids=[c["name"] for c in QC.CASES])
def test_golden_parity_from_host_and_device_pixels(c):
    import torch
    from pixo_amd import jpeg
    px = QC.make_input(c)
    before, fallbacks = png().dither_stats(), jpeg.lookback_fallbacks()
    out = png().encode(px, QC.options(c))
    check_file(c, out)
    assert png().encode_device(torch.from_numpy(px.copy()).cuda(), QC.options(c)) == out
    # The form that carries the W + 2H claim really ran: images of more than one band go through the chained launch, and no
    # band gave up (a give-up would quietly hand the image to the band-by-band launches, H / 64 times as many dependent steps)
    chained, banded, gave_up = (a - b for a, b in zip(png().dither_stats(), before))
    assert gave_up == 0 and jpeg.lookback_fallbacks() == fallbacks
    if c["applied"]:
        assert (chained, banded) == ((2, 0) if c["h"] > 64 else (0, 2))
    else:
        assert (chained, banded) == (0, 0)


@pytest.mark.parametrize("c", QC.DECLINED, ids=[c["name"] for c in QC.DECLINED])
def test_gate_declines_file_is_the_lossless_one(c):
    P, px, o = png(), QC.make_input(c), QC.options(c)
    lossless = QC.options(c)
    lossless.quantization = P.QuantizationOptions()
    assert P.encode(px, o) == P.encode(px, lossless)
    assert not P.quantize(px, o).applied


def force_options(c, max_colors=256, dithering=True, strategy=None):
    from pixo_amd import ColorType
    P = png()
    b = P.PngOptions.builder(c["w"], c["h"]).color_type(ColorType(c["color_type"])).preset(c["preset"]).flags(P.NO_RAYON) \
        .quantization_mode(P.QuantizationMode.FORCE).quantization_max_colors(max_colors).quantization_dithering(dithering)
    if strategy is not None:
        b = b.filter_strategy(strategy)
    return b.build()


def check_against_model(c, max_colors, dithering):
    q = png().quantize(QC.make_input(c), force_options(c, max_colors, dithering))
    palette, idx, rec = QC.model(c, max_colors, dithering)
    assert q.applied
    assert QC.palette_keys(q.palette) == palette
    assert q.trns_len == M.trns_len(palette)
    assert np.array_equal(q.indices, idx)
    return rec


# The options the wasm cannot reach (Force, dithering off, other palette sizes), on at most 20,000 pixels each, and the shapes
# Auto cannot fire on: one pixel, one column, one row, the x + 2 edges.
FORCE = [(QC.force_case(w, h, ct, n, seed), mc, dith) for (w, h, ct, n, seed, mc, dith) in [
    (1, 1, 2, 5, 1, 256, True), (1, 70, 3, 300, 2, 16, True), (70, 1, 2, 300, 3, 16, True), (2, 3, 3, 300, 4, 2, True), (3, 2, 2, 300, 5, 2, True),
    (5, 200, 2, 300, 6, 16, True), (130, 65, 2, 1000, 7, 256, False), (67, 129, 3, 1000, 8, 255, True), (130, 65, 3, 1000, 9, 0, True),
    (130, 65, 2, 1000, 10, 2, True), (67, 129, 2, 4000, 11, 300, False), (130, 65, 3, 300, 12, 16, False), (131, 70, 3, 200, 13, 256, True),
]]


@pytest.mark.parametrize("c,max_colors,dithering", FORCE, ids=["%s_m%d_d%d" % (c["name"], mc, d) for c, mc, d in FORCE])
def test_force_options_against_model(c, max_colors, dithering):
    rec = check_against_model(c, max_colors, dithering)
    if c["n"] <= min(max_colors, 256):
        assert rec["early_out"]  # stride 1: the palette is the image's own colours, every index an exact lookup


def test_explicit_sub_filter_is_kept():
    c = QC.force_case(130, 65, 2, 1000, 7)
    P = png()
    out = P.encode(QC.make_input(c), force_options(c, 256, True, strategy=P.FilterStrategy.SUB))
    _, idx, _ = QC.model(c, 256, True)
    idat, other = PF.parse(out)
    assert zlib.decompress(b"".join(idat)) == M.indexed_stream(idx, c["w"], c["h"], 1)
    none = P.encode(QC.make_input(c), force_options(c, 256, True, strategy=P.FilterStrategy.BIGRAMS))
    assert zlib.decompress(b"".join(PF.parse(none)[0])) == M.indexed_stream(idx, c["w"], c["h"], 0)


@pytest.mark.parametrize("name", ["pal_n1000_67x129_c3_p1", "pal_n1000_512x512_c3_p0"])
def test_chained_and_band_by_band_dither_give_the_same_bytes(name):
    from pixo_amd import _lib
    c = next(c for c in QC.CASES if c["name"] == name)
    px, L = QC.make_input(c), _lib.load()
    s0 = png().dither_stats()
    chained = png().encode(px, QC.options(c))
    s1 = png().dither_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (1, 0, 0), "the default run did not stay in the chained launch"
    try:
        L.pixo_hip_debug_configure(b"spin_budget=0")
        band_by_band = png().encode(px, QC.options(c))
    finally:
        L.pixo_hip_debug_configure(None)  # back to the environment's switches
    s2 = png().dither_stats()
    assert (s2[0] - s1[0], s2[1] - s1[1], s2[2] - s1[2]) == (0, 1, 0), "spin_budget=0 launched the chained form"
    assert band_by_band == chained
    check_file(c, band_by_band)


def test_more_than_8192_sampled_colours_under_force():
    """The one place the source leaves open (an unstable sort cuts the histogram to 8,192): the library's own palette, fed to
    the model's table and mapping stages, reproduces the library's indices; the palette is within max_colors; two runs agree."""
    w, h = 150, 100
    c = dict(gen="many", w=w, h=h, color_type=2, preset=0, seed=1, name="many_150x100")
    px = QC.make_input(c)
    assert len(np.unique(M.keys_of(px, 3))) > 8192
    for max_colors, dithering in ((256, True), (64, False)):
        o = force_options(c, max_colors, dithering)
        q = png().quantize(px, o)
        assert q.applied and 0 < len(q.palette) <= max_colors and int(q.indices.max()) < len(q.palette)
        palette = QC.palette_keys(q.palette)
        lut = M.build_lut(palette)
        px4 = M.rgba(M.keys_of(px, 3))
        want = M.dither(px4, w, h, lut, palette) if dithering else M.lookup_all(px4, lut, palette)
        assert np.array_equal(q.indices, want)
        again = png().quantize(px, o)
        assert again.palette == q.palette and np.array_equal(again.indices, q.indices)
    mp, midx, _ = QC.model(c, 256, True)  # ... and with the stated tie-break (ascending key) the model agrees entirely
    q = png().quantize(px, force_options(c, 256, True))
    assert QC.palette_keys(q.palette) == mp and np.array_equal(q.indices, midx)


def test_quantize_device_leaves_the_indices_in_hbm():
    import torch
    c = next(c for c in QC.CASES if c["name"] == "pal_n1000_257x131_c3_p2")
    px = QC.make_input(c)
    d_idx = torch.zeros(c["w"] * c["h"], dtype=torch.uint8, device="cuda")
    q = png().quantize_device(torch.from_numpy(px.copy()).cuda(), QC.options(c), d_idx)
    palette, idx, _ = QC.model(c)
    assert q.applied and QC.palette_keys(q.palette) == palette and q.trns_len == M.trns_len(palette)
    assert np.array_equal(d_idx.cpu().numpy(), idx)
