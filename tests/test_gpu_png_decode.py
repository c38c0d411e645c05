"""PNG decode on the device against the sequential model (tests/png_decode_model.py, pinned by
tests/test_png_decode_model.py): every colour type and depth at the sizes where the reconstruction kernel's structure can go
wrong (one row, one column, one row more than a wavefront of rows, a run of rows across two pass boundaries), every filter
layout, ragged 16-byte pieces, round trips through the library's own encoders, the device route handed to resize and to the
JPEG encoder without a host synchronisation, call histories, and the refusals only the inflated stream can show."""
import hashlib
import threading

import numpy as np
import pytest

import png_decode_cases as PC
import png_decode_model as M
import png_file_cases as FC
import png_quantize_cases as QC
import synth

pytestmark = pytest.mark.gpu


def lib():
    from pixo_amd import decode
    return decode


def check(png, name=""):
    from pixo_amd import ColorType
    want = PC.model(png)
    assert not isinstance(want, Exception), (name, want)
    im = lib().decode_png(png)
    assert (im.width, im.height, im.color_type) == (want[0], want[1], ColorType(want[3])), name
    assert im.pixels == want[2], "%s: pixels differ from the model's, first at byte %d" % (
        name, next(i for i, (a, b) in enumerate(zip(im.pixels, want[2])) if a != b) if len(im.pixels) == len(want[2]) else -1)
    return im


def shape_params():
    from pixo_amd import _lib  # (the pass height is the kernel's own constant)
    return list(PC.shape_cases(int(_lib.load().pixo_hip_png_unfilter_pass_rows())))


SHAPES = shape_params()
LAYOUTS = list(PC.layout_cases())


@pytest.mark.parametrize("name,png", SHAPES, ids=[n for n, _ in SHAPES])
def test_shape_sweep(name, png):
    check(png, name)


@pytest.mark.parametrize("name,png", LAYOUTS, ids=[n for n, _ in LAYOUTS])
def test_filter_layouts(name, png):
    check(png, name)


def test_filter_unit_8_and_ragged_pieces():
    check(PC.make(40, 40, PC.RGBA, 16, seed=41), "16-bit RGBA 40x40")
    check(PC.make(1000, 3, PC.INDEXED, 1, seed=42, plte_entries=2, trns=bytes([9])), "1-bit palette 1000x3")
    check(PC.make(33, 9, PC.RGB, 8, seed=43, idat_split=50), "many IDAT chunks")


@pytest.mark.parametrize("c", FC.CASES, ids=[c["name"] for c in FC.CASES])
def test_round_trip_through_png_encode(c):
    from pixo_amd import png
    px = FC.make_input(c)
    im = check(png.encode(px, FC.options(c)), c["name"])
    # lossless 8-bit input: the decoded pixels are the original's, whatever colour type the encoder reduced them to
    orig = np.asarray(px, np.uint8).reshape(c["h"] * c["w"], -1)
    got = np.frombuffer(im.pixels, np.uint8).reshape(c["h"] * c["w"], -1)
    assert np.array_equal(to_rgba(got), to_rgba(orig))


def to_rgba(p):
    n, ch = p.shape
    out = np.full((n, 4), 255, np.uint8)
    if ch in (1, 2):
        out[:, 0] = out[:, 1] = out[:, 2] = p[:, 0]
    else:
        out[:, :3] = p[:, :3]
    if ch in (2, 4):
        out[:, 3] = p[:, ch - 1]
    return out


@pytest.mark.parametrize("c", QC.APPLIED[:4], ids=[c["name"] for c in QC.APPLIED[:4]])
def test_round_trip_through_the_lossy_encoder(c):
    from pixo_amd import png
    check(png.encode(QC.make_input(c), QC.options(c)), c["name"])


def test_device_route_feeds_resize_and_jpeg_without_a_host_wait():
    import torch
    from pixo_amd import ColorType, jpeg, resize
    w, h = 129, 130
    file = PC.make(w, h, PC.RGB, 8, seed=51)
    pixels = np.frombuffer(PC.model(file)[2], np.uint8)
    ropts = resize.ResizeOptions.builder(w, h).dst(64, 48).color_type(ColorType.Rgb).algorithm(resize.ResizeAlgorithm.Lanczos3).build()
    jopts = jpeg.JpegOptions.builder(w, h).color_type(ColorType.Rgb).quality(80).subsampling(jpeg.Subsampling.S420).build()
    want_small, want_jpeg = resize.resize(pixels, ropts), jpeg.encode(pixels, jopts)
    side = torch.cuda.Stream()
    before = jpeg.get_producer_stream()
    try:
        with torch.cuda.stream(side):
            jpeg.set_producer_stream(side.cuda_stream)
            d_small = torch.empty(64 * 48 * 3, dtype=torch.uint8, device="cuda")
            d_px, ct = lib().decode_png_device(file, stream=side.cuda_stream)
            resize.resize_device(d_px, ropts, d_small, side.cuda_stream)
            got_jpeg = jpeg.encode_device(d_px, jopts)  # (ordered behind the producer stream by the library)
            side.synchronize()
    finally:
        jpeg.set_producer_stream(before)
    assert ct == ColorType.Rgb and d_px.shape == (h, w, 3)
    assert d_small.cpu().numpy().tobytes() == want_small and got_jpeg == want_jpeg


def test_too_small_a_capacity_says_what_is_needed():
    import torch
    from pixo_amd import error
    file = PC.make(20, 10, PC.RGBA, 8, seed=52)
    with pytest.raises(error.BufferTooSmall) as e:
        lib().decode_png_device(file, out=torch.empty(799, dtype=torch.uint8, device="cuda"))
    assert e.value.needed == 800 and str(e.value) == "output buffer too small: need 800 bytes"
    out = torch.empty(800, dtype=torch.uint8, device="cuda")
    t, _ = lib().decode_png_device(file, out=out)
    assert t.cpu().numpy().tobytes() == PC.model(file)[2]


def test_buffers_regrow_across_calls():
    for (w, h, ct, d, seed) in [(300, 200, PC.RGB, 8, 61), (3, 2, PC.GRAY, 2, 62), (310, 260, PC.RGBA, 16, 63), (5, 5, PC.INDEXED, 8, 64)]:
        check(PC.make(w, h, ct, d, seed=seed), "%dx%d c%d d%d" % (w, h, ct, d))


def test_three_threads_decode_different_files():
    files = [PC.make(90, 140, PC.RGB, 8, seed=71), PC.make(77, 150, PC.INDEXED, 2, seed=72, trns=bytes([3])), PC.make(64, 129, PC.GRAY_ALPHA, 16, seed=73)]
    want = [PC.model(f) for f in files]
    errors = []

    def work(i):
        try:
            for _ in range(3):
                im = lib().decode_png(files[i])
                assert (im.width, im.height, im.pixels, int(im.color_type)) == want[i]
        except BaseException as e:  # noqa: BLE001
            errors.append((i, e))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_refusals_only_the_stream_can_show_and_the_context_survives():
    from pixo_amd import error
    h = 9
    good = PC.make(11, h, PC.RGB, 8, seed=81)
    bad = {
        "row0": [5] + [1] * (h - 1),
        "last_row": [2] * (h - 1) + [5],
        "two_rows": [0, 0, 7, 0, 0, 6, 0, 0, 0],  # the first offending row decides
    }
    files = {k: PC.make(11, h, PC.RGB, 8, filters=f, seed=82) for k, f in bad.items()}
    files["missing_plte"] = PC.make(11, h, PC.INDEXED, 4, seed=83, no_plte=True)
    files["filter_before_missing_plte"] = PC.make(11, h, PC.INDEXED, 4, filters=[0] * (h - 1) + [9], seed=84, no_plte=True)
    for name, f in files.items():
        want = PC.model(f)
        assert isinstance(want, M.DecodeError), name
        with pytest.raises(error.InvalidDecode) as e:
            lib().decode_png(f)
        assert str(e.value) == str(want), name
        check(good, "after " + name)
    assert str(PC.model(files["two_rows"])) == "Decode error: invalid filter type: 7"


def test_one_wide_image_through_our_encoder():
    from pixo_amd import ColorType, png
    w, h = 4096, 64
    rgb = synth.scene(w, h, 5).reshape(h * w, 3)
    px = np.concatenate([rgb, (rgb[:, :1] // 2 + 100).astype(np.uint8)], axis=1)
    o = png.PngOptions.builder(w, h).color_type(ColorType.Rgba).preset(1).flags(png.NO_RAYON).build()
    file = png.encode(px, o)
    want = PC.model(file)
    im = lib().decode_png(file)
    assert hashlib.sha256(im.pixels).digest() == hashlib.sha256(want[2]).digest()
    assert im.pixels == px.tobytes() or int(im.color_type) != 3  # (kept as RGBA: the original pixels)
