"""GPU parity of the PNG prepare path (pixo_hip_png_prepare*, png_reduce.hip + png_filter.hip): every vector the reference's
own wasm build made, byte for byte through host and device entries (stream, layout, Adler-32), seeded random cases against
the model (tests/png_reduce_model.py), and the path's place in a resident pipeline.  -m gpu."""
import threading

import numpy as np
import pytest

import oracle_lib as O
import png_reduce_cases as PC
import png_reduce_model as M
import resize_cases as RC
import resize_model as RM
from pixo_amd import ColorType, _lib, error, jpeg, png, resize

pytestmark = pytest.mark.gpu

_torch = None


def torch():
    global _torch
    if _torch is None:
        import torch as t
        _torch = t
    return _torch


def preset_options(c):
    # the wasm build has no `parallel` feature: its AdaptiveFast (preset 0) is the stateful one
    return png.PngOptions.builder(c["w"], c["h"]).color_type(ColorType(c["color_type"])).preset(c["preset"]).flags(png.NO_RAYON).build()


def device_prepare(px, o, offset=0):
    """prepare_device with canary bytes around d_out and behind the stream -> (stream, layout dict, adler)"""
    t = torch()
    d_px = t.from_numpy(np.ascontiguousarray(px)).to("cuda:0")
    cap = o.full_size()
    d_all = t.full((cap + offset + 64,), 0xA5, dtype=t.uint8, device="cuda:0")
    d_out = d_all[offset:offset + cap]
    t.cuda.synchronize()
    n, lay, adler = png.prepare_device(d_px, o, d_out)
    t.cuda.synchronize()
    got = d_all.cpu().numpy()
    assert n <= cap
    assert (got[:offset] == 0xA5).all() and (got[offset + n:] == 0xA5).all(), "bytes outside the stream were written"
    return got[offset:offset + n], M.layout_of(lay), adler


@pytest.mark.parametrize("c", PC.CASES, ids=[c["name"] for c in PC.CASES])
def test_reference_made_vectors_host_pixels(c):
    stream, lay, adler = png.prepare(PC.make_input(c), preset_options(c))
    PC.check(c, stream, M.layout_of(lay), adler)


@pytest.mark.parametrize("c", PC.CASES, ids=[c["name"] for c in PC.CASES])
def test_reference_made_vectors_device_pixels(c):
    stream, lay, adler = device_prepare(PC.make_input(c), preset_options(c), offset=16 * (c["seed"] % 2))
    PC.check(c, stream, lay, adler)


def test_random_cases_against_the_model():
    bad = []
    for seed in range(320):
        px, w, h, ct, sw, strategy, flags = PC.random_case(seed)
        want, wlay, wad = M.prepare(px, w, h, ct, M.Opts(strategy, sw["optimize_alpha"], sw["reduce_color_type"], sw["reduce_palette"], flags))
        o = png.PngOptions.builder(w, h).color_type(ColorType(ct)).filter_strategy(png.FilterStrategy(strategy)).flags(flags) \
            .optimize_alpha(sw["optimize_alpha"]).reduce_color_type(sw["reduce_color_type"]).reduce_palette(sw["reduce_palette"]).build()
        if seed % 2:
            got, lay, ad = png.prepare(px, o)
            lay = M.layout_of(lay)
        else:
            got, lay, ad = device_prepare(px, o)
        if lay != wlay or ad != wad or not np.array_equal(got, want):
            bad.append("seed %d %dx%d ct %d %s strategy %d: layout %s want %s, adler %08x want %08x" % (
                seed, w, h, ct, sw, strategy, {k: v for k, v in lay.items() if k != "palette"}, {k: v for k, v in wlay.items() if k != "palette"}, ad, wad))
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("ct", [0, 1, 2, 3])
def test_switches_off_is_the_filter_entry(ct):
    t = torch()
    for (w, h, strategy, flags) in [(300, 70, 6, 0), (64, 64, 7, 0), (333, 33, 7, 1), (97, 40, 8, 0), (50, 20, 4, 0)]:
        spp = ColorType(ct).bytes_per_pixel()
        px = np.random.RandomState(w + ct).randint(0, 4, w * h * spp).astype(np.uint8)  # few colours, alpha 0 among them: nothing may act
        o = png.PngOptions.builder(w, h).color_type(ColorType(ct)).filter_strategy(png.FilterStrategy(strategy)).flags(flags).build()
        d_px = t.from_numpy(px).to("cuda:0")
        d_ref = t.empty(o.full_size(), dtype=t.uint8, device="cuda:0")
        t.cuda.synchronize()
        wad = png.apply_filters_device(d_px, w, h, spp, d_ref, strategy, flags)
        want = d_ref.cpu().numpy()
        got, lay, ad = device_prepare(px, o)
        assert np.array_equal(got, want) and ad == wad
        assert (lay["color_type_byte"], lay["bit_depth"], lay["bytes_per_pixel"], lay["row_bytes"], lay["palette"]) == (M.PNG_CT[ct], 8, spp, w * spp, [])
        got, _, ad = png.prepare(px, o)
        assert np.array_equal(got, want) and ad == wad


def test_short_buffer_reports_the_length():
    import ctypes as C
    c = next(c for c in PC.CASES if c["name"].startswith("pal_aopaque_n5_pnoise_80x70"))
    px, o = PC.make_input(c), preset_options(c).to_c()
    L = _lib.load()
    lay, n, ad = _lib.PngLayoutC(), C.c_size_t(), C.c_uint32()
    out = np.zeros(c["filtered_len"] - 1, np.uint8)
    assert L.pixo_hip_png_prepare(px.ctypes.data, px.size, C.byref(o), out.ctypes.data, out.size, C.byref(n), C.byref(lay), C.byref(ad)) == -9
    assert n.value == c["filtered_len"] and (out == 0).all()
    with pytest.raises(error.InvalidDimensions):
        png.prepare(px, png.PngOptions.builder(0, 3).build())


def test_pipeline_resize_then_prepare_on_one_stream():
    """resize_device -> png.prepare_device on the same stream, no host copy of the resized pixels: equals the model's
    prepared stream of the (model-checked) resized pixels.  Once with content that stays RGBA, once reduced to few colours."""
    t = torch()
    c = next(c for c in RC.ok_cases() if c["name"].startswith("nearest_160x120_to_61x47_c2"))
    for levels in (256, 3):
        px = (RC.make_input(c).astype(np.uint32) * levels // 256 * (255 // max(levels - 1, 1))).astype(np.uint8)
        want_px = np.frombuffer(RM.resize(px, c["sw"], c["sh"], c["dw"], c["dh"], 3, c["algorithm"]), np.uint8)
        o = png.PngOptions.builder(c["dw"], c["dh"]).color_type(ColorType.Rgb).preset(1).build()
        ro = resize.ResizeOptions.builder(c["sw"], c["sh"]).dst(c["dw"], c["dh"]).color_type(ColorType.Rgb) \
            .algorithm(resize.ResizeAlgorithm(c["algorithm"])).build()
        s = t.cuda.Stream()
        with t.cuda.stream(s):
            d_src = t.from_numpy(px).to("cuda:0")
            d_dst = t.empty(c["len"], dtype=t.uint8, device="cuda:0")
            d_out = t.empty(o.full_size(), dtype=t.uint8, device="cuda:0")
        with jpeg.producer_stream(s.cuda_stream):
            resize.resize_device(d_src, ro, d_dst, s.cuda_stream)
            n, lay, adler = png.prepare_device(d_dst, o, d_out)
        t.cuda.synchronize()
        want, wlay, wad = M.prepare(want_px, c["dw"], c["dh"], 2, M.Opts.preset(1))
        assert M.layout_of(lay) == wlay and adler == wad and np.array_equal(d_out.cpu().numpy()[:n], want)
        assert (levels == 3) == (wlay["color_type_byte"] == 3)


def test_two_calling_threads():
    cases = [c for c in PC.small(200 * 200)]
    errors = []

    def work(k):
        try:
            for rep in range(2):
                for c in cases[k::2]:
                    stream, lay, adler = png.prepare(PC.make_input(c), preset_options(c))
                    PC.check(c, stream, M.layout_of(lay), adler)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert not any(th.is_alive() for th in threads), "a calling thread did not finish"
    assert not errors, errors[:3]


def test_trim_then_again():
    small = next(c for c in PC.CASES if c["name"].startswith("pal_asome_n17_ppopular_71x67"))
    large = next(c for c in PC.CASES if (c["w"], c["h"]) == (1920, 1080))
    for c in (small, large, small):
        stream, lay, adler = png.prepare(PC.make_input(c), preset_options(c))
        PC.check(c, stream, M.layout_of(lay), adler)
    assert _lib.load().pixo_hip_trim() == 0
    for c in (small, large):
        stream, lay, adler = device_prepare(PC.make_input(c), preset_options(c))
        PC.check(c, stream, lay, adler)
    assert _lib.load().pixo_hip_trim() == 0
    stream, lay, adler = png.prepare(PC.make_input(small), preset_options(small))
    PC.check(small, stream, M.layout_of(lay), adler)
