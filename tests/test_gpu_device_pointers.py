"""Every PNG, zlib and decode device entry handed caller pointers of every alignment (include/pixo_hip.h asks for none): the
launchers choose a kernel variant from the pointer's low bits, and a fresh allocation only ever reaches the vector one.
Inputs and outputs are views into larger buffers (tests/device_pointer_cases.py) with canary bytes on both sides; a capacity is
exactly the bytes needed.  Every result is compared with the stage's independent reference (PNG oracle, the models, Python's
zlib, the host entry whose stream is audited token by token), never with an aligned run of the same code.  The tables' claims
are pinned without a GPU by tests/test_device_pointer_cases_cpu.py.  -m gpu."""
import io
import zlib

import numpy as np
import pytest

import device_pointer_cases as DP
import oracle_lib as O
import png_decode_cases as PC
import png_file_cases as FC
import png_quantize_cases as QC
import png_quantize_model as QM
import png_reduce_model as RM

pytestmark = pytest.mark.gpu


def png():
    from pixo_amd import png as P
    return P


def first_difference(got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.size != want.size:
        return "lengths %d and %d" % (got.size, want.size)
    at = np.flatnonzero(got != want)
    return "equal" if at.size == 0 else "first differing byte %d: got %d, want %d (%d differ)" % (at[0], got[at[0]], want[at[0]], at.size)


# ---- A. png.apply_filters_device against the oracle --------------------------------------------------------------------------
FILTER_PARAMS = [(c, s) for c in DP.FILTER_CASES for s in c["strategies"]]
_FILTER_INPUT = {}


def filter_input(c):
    if c["name"] not in _FILTER_INPUT:
        px = DP.filter_content(c["w"], c["h"], c["bpp"], 1)
        px.setflags(write=False)
        _FILTER_INPUT[c["name"]] = px
    return _FILTER_INPUT[c["name"]]


@pytest.mark.parametrize("c,strategy", FILTER_PARAMS, ids=["%s_s%d" % (c["name"], s) for c, s in FILTER_PARAMS])
def test_filters_at_every_alignment(c, strategy):
    import torch
    w, h, bpp = c["w"], c["h"], c["bpp"]
    px = filter_input(c)
    want, wad = O.png_filter(px, w, h, bpp, strategy, stateful_fast=c["stateful"])
    assert wad == zlib.adler32(want.tobytes())
    n = png().filtered_size(w, h, bpp)
    for (i, o) in c["pairs"]:
        d_in_all, d_in = DP.at_offset(px, i)
        d_out_all, d_out = DP.at_offset(n, o)
        adler = png().apply_filters_device(d_in, w, h, bpp, d_out, png().FilterStrategy(strategy))
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert np.array_equal(got, want), "offsets (%d, %d): %s" % (i, o, first_difference(got, want))
        assert adler == wad, (i, o)
        assert DP.untouched(d_out_all, o, n), "offsets (%d, %d): bytes around the stream were written" % (i, o)
        assert np.array_equal(d_in.cpu().numpy(), px) and DP.untouched(d_in_all, i, px.size), "the input was written"


# ---- B. png.prepare_device against the model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", DP.REDUCE_CASES, ids=[c["name"] for c in DP.REDUCE_CASES])
def test_prepare_at_every_alignment(c):
    import torch
    px = DP.reduce_input(c)
    for key in c["outcomes"]:
        want, wlay, wad = RM.prepare(px, c["w"], c["h"], c["ct"], DP.reduce_model_options(key))
        o = DP.reduce_options(c, key)
        cap = o.full_size()
        for i in DP.REDUCE_IN_OFFSETS:
            out_off = DP.OUT_FOR[i]
            d_in_all, d_in = DP.at_offset(px, i)
            d_out_all, d_out = DP.at_offset(cap, out_off)
            n, lay, adler = png().prepare_device(d_in, o, d_out)
            torch.cuda.synchronize()
            where = "%s, offsets (%d, %d)" % (key, i, out_off)
            assert RM.layout_of(lay) == wlay, where
            assert n == want.size <= cap and adler == wad, where
            got = d_out_all.cpu().numpy()[DP.PAD + out_off:]
            assert np.array_equal(got[:n], want), "%s: %s" % (where, first_difference(got[:n], want))
            assert (got[n:] == DP.FILL).all() and DP.untouched(d_out_all, out_off, cap), "%s: bytes outside the stream were written" % where
            assert np.array_equal(d_in.cpu().numpy(), px) and DP.untouched(d_in_all, i, px.size), "the input was written"


# ---- C. png.quantize_device and the lossy file against the model -------------------------------------------------------------
def force_options(q):
    from pixo_amd import ColorType
    P, c = png(), q["c"]
    return P.PngOptions.builder(c["w"], c["h"]).color_type(ColorType(c["color_type"])).preset(c["preset"]).flags(P.NO_RAYON) \
        .quantization_mode(P.QuantizationMode.FORCE).quantization_max_colors(q["max_colors"]).quantization_dithering(q["dithering"]).build()


@pytest.mark.parametrize("q", DP.QUANT_CASES, ids=[q["c"]["name"] for q in DP.QUANT_CASES])
def test_quantize_at_every_alignment(q):
    import torch
    from pixo_amd import jpeg
    P, c = png(), q["c"]
    px, o = QC.make_input(c), force_options(q)
    palette, idx, rec = QC.model(c, q["max_colors"], q["dithering"])
    assert rec["early_out"] == q["early_out"]
    file = P.encode(px, o)  # (pinned to the reference's vectors by test_gpu_png_quantize.py)
    pixels = c["w"] * c["h"]
    for i in DP.QUANT_IN_OFFSETS:
        out_off = DP.OUT_FOR[i]
        d_in_all, d_in = DP.at_offset(px, i)
        d_idx_all, d_idx = DP.at_offset(pixels, out_off)
        before, fallbacks = P.dither_stats(), jpeg.lookback_fallbacks()
        got = P.quantize_device(d_in, o, d_idx)
        torch.cuda.synchronize()
        chained, banded, gave_up = (a - b for a, b in zip(P.dither_stats(), before))
        where = "offsets (%d, %d)" % (i, out_off)
        assert gave_up == 0 and jpeg.lookback_fallbacks() == fallbacks, where
        assert (chained, banded) == {"chained": (1, 0), "banded": (0, 1), None: (0, 0)}[q["form"]], where
        assert got.applied and QC.palette_keys(got.palette) == palette and got.trns_len == QM.trns_len(palette), where
        indices = d_idx.cpu().numpy()
        assert np.array_equal(indices, idx), "%s: %s" % (where, first_difference(indices, idx))
        assert DP.untouched(d_idx_all, out_off, pixels), "%s: bytes around the indices were written" % where
        assert P.encode_device(d_in, o) == file, where
        assert np.array_equal(d_in.cpu().numpy(), px) and DP.untouched(d_in_all, i, px.size), "the input was written"


# ---- D. png.zlib_compress_device -----------------------------------------------------------------------------------------------
ZLIB = DP.zlib_cases()


@pytest.mark.parametrize("effort", [0, 1])
@pytest.mark.parametrize("name,data,bpp,row,shrinks", ZLIB, ids=[z[0] for z in ZLIB])
def test_zlib_at_every_alignment(name, data, bpp, row, shrinks, effort):
    import torch
    P = png()
    want = P.zlib_compress(data, 6, bpp, row, effort)  # the host entry: the audited stream
    assert zlib.decompress(want) == data
    cap = P.stored_bound(len(data))
    for (i, o) in DP.IN_OUT:
        d_in_all, d_in = DP.at_offset(data, i)
        d_out_all, d_out = DP.at_offset(cap, o)
        n = P.zlib_compress_device(d_in, len(data), d_out, cap, 6, bpp, row, effort)
        torch.cuda.synchronize()
        where = "offsets (%d, %d)" % (i, o)
        assert n <= cap, where
        got = d_out_all.cpu().numpy()[DP.PAD + o:]
        assert zlib.decompress(got[:n].tobytes()) == data, where
        assert got[:n].tobytes() == want, "%s: %s" % (where, first_difference(got[:n], np.frombuffer(want, np.uint8)))
        assert (got[n:] == DP.FILL).all() and DP.untouched(d_out_all, o, cap), "%s: bytes outside the stream were written" % where
        assert DP.untouched(d_in_all, i, len(data)), "the input's surroundings were written"
    if shrinks:
        assert len(want) < len(data)


# ---- E. decode.decode_png_device(out=view) against the model -----------------------------------------------------------------
@pytest.mark.parametrize("d", DP.DECODE_CASES, ids=[d["name"] for d in DP.DECODE_CASES])
def test_decode_into_every_alignment(d):
    import torch
    from pixo_amd import ColorType, decode
    w, h, pixels, ct = PC.model(d["file"])
    want = np.frombuffer(pixels, np.uint8)
    for o in DP.DECODE_OUT_OFFSETS:
        d_all, d_out = DP.at_offset(want.size, o)  # capacity: exactly the pixels
        t, color = decode.decode_png_device(d["file"], out=d_out)
        torch.cuda.synchronize()
        assert color == ColorType(ct) and tuple(t.shape) == (h, w, d["out_bpp"]) and t.data_ptr() == d_out.data_ptr()
        got = d_out.cpu().numpy()
        assert np.array_equal(got, want), "offset %d: %s" % (o, first_difference(got, want))
        assert DP.untouched(d_all, o, want.size), "offset %d: bytes around the pixels were written" % o


# ---- F. png.encode_device, lossless whole files ------------------------------------------------------------------------------
FILES = DP.file_cases()


@pytest.mark.parametrize("c", FILES, ids=[c["name"] for c in FILES])
def test_lossless_file_from_pixels_at_every_alignment(c):
    from PIL import Image
    P = png()
    px = np.ascontiguousarray(FC.make_input(c), np.uint8).reshape(-1)
    want = P.encode(px, FC.options(c))
    spp = DP.SPP[c["color_type"]]
    for i in DP.FILE_IN_OFFSETS:
        d_all, d_in = DP.at_offset(px, i)
        got = P.encode_device(d_in, FC.options(c))
        assert got == want, "offset %d: %s" % (i, first_difference(np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)))
        assert np.array_equal(d_in.cpu().numpy(), px) and DP.untouched(d_all, i, px.size), "the input was written"
    im = Image.open(io.BytesIO(want))
    mode = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[spp]
    seen, orig = np.asarray(im.convert(mode)).reshape(-1, spp).copy(), px.reshape(-1, spp).copy()
    if spp in (2, 4) and FC.options(c).optimize_alpha:  # the one lossy step: colour under alpha 0 is cleared
        seen[orig[:, -1] == 0, :-1] = 0
        orig[orig[:, -1] == 0, :-1] = 0
    assert np.array_equal(seen, orig), "Pillow reads other pixels from the file"
