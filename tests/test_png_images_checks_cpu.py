"""CPU-only: the PNG encode entries for images of individual sizes (pixo_hip_png_encode_images*): symbols, route bits, the
argument checks in the documented order — status and exact pixo_hip_last_error() text, " (image i)" included; every check runs
before the thread's context is touched — and the plan (sub-batches, way in, resolved strategy, filter launches) against values
worked out here.
Order: null options, unknown strategy, null pixels, null images, batch in 1..65535, the quantisation struct when given, null
files / offsets, null lens, then image by image: zero side, side above 2^24, colour type above 3, offset + bytes beyond 2^62;
the host entry last: data_len below the furthest image's end."""
import ctypes as C
import os
import re

import pytest

from pixo_amd import ColorType, _lib, decode, error, jpeg, png, resize
from test_entry_checks_cpu import BUF, COLOUR, COMPRESSION, DIMS, LARGE, LENGTH, MAX, P, STRATEGY, UNSUPPORTED, dims, large, last_error, length, null, run
from test_png_batch_checks_cpu import BATCH, bad_mode_text, quantization

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NAMES = ("pixo_hip_png_encode_images_device", "pixo_hip_png_encode_images_device_into", "pixo_hip_png_encode_images",
         "pixo_hip_debug_png_encode_images_plan")
TOO_FAR = "Compression error: batch input too large"


def test_symbols_are_declared_listed_and_exported():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pixo_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name


def test_route_bits_are_new_and_the_pinned_dicts_are_unchanged():
    routes = open(os.path.join(ROOT, "pixo_amd", "csrc", "routes.hpp")).read()
    assert re.search(r"\bPNG_IMAGES = 1ull << 45,", routes) and re.search(r"\bPNG_IMAGES_FILTER = 1ull << 46,", routes)
    assert png.IMAGES_ROUTES == {"PNG_IMAGES": 45, "PNG_IMAGES_FILTER": 46}
    assert (png.ROUTE_PNG_IMAGES, png.ROUTE_PNG_IMAGES_FILTER) == (1 << 45, 1 << 46)
    assert png.ROUTES == {"PNG_BATCH": 39, "PNG_BATCH_FILTER": 40, "SUB_BATCHES": 26}
    assert max(jpeg.ROUTES.values()) < 42
    taken = set(png.ROUTES.values()) | set(jpeg.ROUTES.values()) | set(decode.ROUTES.values()) | set(decode.INFLATE_ROUTES.values()) | set(resize.ROUTES.values())
    assert not taken & {45, 46}


def images_c(*rows):
    """rows of (width, height, colour type, offset)"""
    arr = (_lib.PngImageC * max(len(rows), 1))()
    for i, (w, h, ct, at) in enumerate(rows):
        arr[i].width, arr[i].height, arr[i].color_type, arr[i].offset = w, h, ct, at
    return arr


GOOD = ((4, 4, 3, 0), (5, 3, 0, 64))  # 64 bytes at 0, 15 bytes at 64: the block ends at 79


def options_c(strategy=7, w=0, h=0, ct=9):
    """(width 0, height 0 and a colour type that is none: the template's own are not read)"""
    return _lib.PngOptionsC(w, h, ct, strategy, 0, 0, 0, 2, 0, 0, 0)


def shared_rows(sink):
    q_rc, q_text = bad_mode_text()
    bad_q = quantization(mode=9)
    far = 1 << 62
    return [
        (dict(o=None, strategy=9), COMPRESSION, null("options")),
        (dict(strategy=9, pixels=None), COMPRESSION, STRATEGY),  # the strategy before the pixels
        (dict(pixels=None, images=None), COMPRESSION, null("pixels")),  # pixels before images
        (dict(images=None, batch=0), COMPRESSION, null("images")),  # images before batch
        (dict(batch=0, q=C.byref(bad_q)), COMPRESSION, BATCH),  # batch before the quantisation
        (dict(batch=65536), COMPRESSION, BATCH),
        (dict(q=C.byref(bad_q), **{sink: None}), q_rc, q_text),  # the quantisation before the sink
        (dict(**{sink: None}, lens=None), COMPRESSION, null(sink)),  # files / offsets before lens
        (dict(lens=None, images=((0, 4, 3, 0),), batch=1), COMPRESSION, null("lens")),  # lens before the images' own
        (dict(images=((4, 4, 3, 0), (0, MAX + 1, 9, far)), batch=2), DIMS, dims(0, MAX + 1) + " (image 1)"),  # a zero side first
        (dict(images=((4, 0, 3, 0), (0, 4, 3, 0)), batch=2), DIMS, dims(4, 0) + " (image 0)"),  # the lowest index decides
        (dict(images=((MAX + 1, 1, 9, far),), batch=1), LARGE, large(MAX + 1, 1) + " (image 0)"),  # too large before the colour type
        (dict(images=((4, 4, 3, 0), (4, 4, 3, 0), (1, MAX + 1, 2, 0)), batch=3), LARGE, large(1, MAX + 1) + " (image 2)"),
        (dict(images=((4, 4, 4, far),), batch=1), COLOUR, UNSUPPORTED + " (image 0)"),  # the colour type before the offset
        (dict(images=((4, 4, 3, 0), (4, 4, 255, 0)), batch=2), COLOUR, UNSUPPORTED + " (image 1)"),
        (dict(images=((4, 4, 3, far - 63),), batch=1), COMPRESSION, TOO_FAR + " (image 0)"),  # 64 bytes: one beyond 2^62
        (dict(images=((4, 4, 3, 0), (4, 4, 3, (1 << 64) - 8)), batch=2), COMPRESSION, TOO_FAR + " (image 1)"),  # (no wrap)
    ]


def entry(fn):
    def call(o=(), strategy=7, images=GOOD, batch=None, **kw):
        oc = options_c(strategy) if o is not None else None
        arr = images_c(*images) if images is not None else None
        n = batch if batch is not None else (len(images) if images is not None else 2)
        return fn(C.byref(oc) if oc is not None else None, arr, n, **kw)
    return call


def test_png_encode_images_device():
    L = _lib.load()
    files, lens = (C.POINTER(C.c_uint8) * 3)(), (C.c_size_t * 3)()

    @entry
    def call(o, images, batch, pixels=P, q=None, files=files, lens=lens):
        return L.pixo_hip_png_encode_images_device(pixels, images, batch, o, q, files, lens)

    run(shared_rows("files"), call)
    assert not files[0] and not files[1] and lens[0] == 0


def test_png_encode_images_device_into():
    L = _lib.load()
    offsets, lens = (C.c_size_t * 3)(), (C.c_size_t * 3)()

    @entry
    def call(o, images, batch, pixels=P, q=None, arena=P, cap=4096, offsets=offsets, lens=lens):
        return L.pixo_hip_png_encode_images_device_into(pixels, images, batch, o, q, arena, cap, offsets, lens)

    run(shared_rows("offsets") + [
        (dict(pixels=None, arena=None, cap=0), COMPRESSION, null("pixels")),  # a size query is checked like any call
    ], call)
    assert bytes(BUF) == bytes(4096), "a refused call wrote into the arena"


def test_png_encode_images_host():
    L = _lib.load()
    files, lens = (C.POINTER(C.c_uint8) * 3)(), (C.c_size_t * 3)()

    @entry
    def call(o, images, batch, pixels=P, n=79, q=None, files=files, lens=lens):
        return L.pixo_hip_png_encode_images(pixels, n, images, batch, o, q, files, lens)

    run(shared_rows("files") + [
        (dict(n=78), LENGTH, length(79, 78)),  # the furthest image's end
        (dict(n=0), LENGTH, length(79, 0)),
        (dict(images=((5, 3, 0, 64), (4, 4, 3, 0)), n=70), LENGTH, length(79, 70)),  # ... whichever image it is
        (dict(images=((4, 4, 3, 0), (4, 0, 3, 0)), n=1), DIMS, dims(4, 0) + " (image 1)"),  # the images' own before the length
        (dict(n=78, lens=None), COMPRESSION, null("lens")),
    ], call)
    assert not files[0] and not files[1] and lens[0] == 0


def test_png_encode_images_plan_checks():
    L = _lib.load()
    sub_first, subs, way, strat, launches = (C.c_uint32 * 4)(), C.c_uint32(), (C.c_uint8 * 3)(), (C.c_uint8 * 3)(), C.c_uint32()

    @entry
    def call(o, images, batch, q=None, align=0, sub_first=sub_first, sub_count=C.byref(subs), way_in=way, run_strategy=strat,
             filter_launches=C.byref(launches)):
        return L.pixo_hip_debug_png_encode_images_plan(images, batch, o, q, align, sub_first, sub_count, way_in, run_strategy, filter_launches)

    q_rc, q_text = bad_mode_text()
    bad_q = quantization(mode=9)
    run([
        (dict(o=None, strategy=9), COMPRESSION, null("options")),
        (dict(strategy=9, images=None), COMPRESSION, STRATEGY),
        (dict(images=None, batch=0), COMPRESSION, null("images")),
        (dict(batch=0, q=C.byref(bad_q)), COMPRESSION, BATCH),
        (dict(q=C.byref(bad_q), align=16), q_rc, q_text),
        (dict(align=16, sub_first=None), COMPRESSION, "Compression error: alignment must be 0..15"),
        (dict(sub_first=None, sub_count=None), COMPRESSION, null("sub_first")),
        (dict(sub_count=None, way_in=None), COMPRESSION, null("sub_count")),
        (dict(way_in=None, run_strategy=None), COMPRESSION, null("way_in")),
        (dict(run_strategy=None, filter_launches=None), COMPRESSION, null("run_strategy")),
        (dict(filter_launches=None, images=((0, 1, 0, 0),), batch=1), COMPRESSION, null("filter_launches")),
        (dict(images=((4, 4, 3, 0), (0, 1, 0, 0)), batch=2), DIMS, dims(0, 1) + " (image 1)"),
    ], call)


def test_errors_raise_their_classes_through_the_wrappers():
    o = png.PngOptions.builder(0, 0).build()
    with pytest.raises(error.InvalidDimensions) as e:
        png.encode_images_plan([(4, 4, ColorType.Rgba, 0), (0, 7, ColorType.Gray, 64)], o)
    assert str(e.value) == dims(0, 7) + " (image 1)"
    with pytest.raises(error.ImageTooLarge) as e:
        png.encode_images_plan([(MAX + 1, 7, ColorType.Gray, 0)], o)
    assert str(e.value) == large(MAX + 1, 7) + " (image 0)"
    with pytest.raises(error.CompressionError) as e:
        png.encode_images_plan([(4, 4, ColorType.Rgba, 1 << 62)], o)
    assert str(e.value) == TOO_FAR + " (image 0)"
    with pytest.raises(error.CompressionError) as e:
        png.encode_images_plan([], o)
    assert str(e.value) == BATCH
    with pytest.raises(error.InvalidDataLength) as e:
        png.encode_images(bytes(78), [(4, 4, ColorType.Rgba, 0), (5, 3, ColorType.Gray, 64)], o)
    assert str(e.value) == length(79, 78)
    arr = images_c((4, 4, 4, 0))
    with pytest.raises(error.UnsupportedColorType) as e:
        png.encode_images_plan(arr, o)
    assert str(e.value) == UNSUPPORTED + " (image 0)"


# ---- the plan ----------------------------------------------------------------------------------------------------------------

S = png.FilterStrategy
RGB, RGBA, GRAY, GA = ColorType.Rgb, ColorType.Rgba, ColorType.Gray, ColorType.GrayAlpha


def opts(strategy=S.ADAPTIVE, flags=0, preset=None):
    b = png.PngOptions.builder(0, 0)  # (a width of 0 in the template: accepted, the records carry the sizes)
    if preset is not None:
        b = b.preset(preset)
    else:
        b = b.filter_strategy(strategy)
    return b.flags(flags).build()


def back_to_back(shapes):
    """(width, height, colour type) -> records at offsets rounded up to 16, as a decode batch lays them out"""
    out, at = [], 0
    for w, h, ct in shapes:
        out.append((w, h, ct, at))
        at += (w * h * ct.bytes_per_pixel() + 15) & ~15
    return out


def test_the_template_options_own_size_is_not_read():
    o = opts()
    assert (o.width, o.height) == (0, 0)
    p = png.encode_images_plan(back_to_back([(8, 8, RGB)]), o)
    assert p == {"sub_first": [0, 1], "way_in": [True], "run_strategy": [S.SUB], "filter_launches": 1}


def test_plan_way_in_and_strategy_at_png_plans_boundaries():
    # area 4096 and 4097 (64 x 64, 241 x 17 = 4097), height 32 and 33
    shapes = [(64, 64, RGB), (241, 17, RGB), (200, 32, RGBA), (200, 33, RGBA), (1, 1, GRAY)]
    recs = back_to_back(shapes)
    p = png.encode_images_plan(recs, opts(S.ADAPTIVE))
    assert p["run_strategy"] == [S.SUB, S.ADAPTIVE, S.ADAPTIVE, S.ADAPTIVE, S.SUB] and p["way_in"] == [True] * 5
    p = png.encode_images_plan(recs, opts(S.BIGRAMS))
    assert p["run_strategy"] == [S.SUB, S.BIGRAMS, S.BIGRAMS, S.BIGRAMS, S.SUB] and p["way_in"] == [True] * 5
    p = png.encode_images_plan(recs, opts(S.MINSUM))  # (not one of the three the small-image rule names)
    assert p["run_strategy"] == [S.MINSUM] * 5 and p["way_in"] == [True] * 5
    # AdaptiveFast: Sub under the area rule (batched); sequential with a height of at most 32 (by itself); batched above
    p = png.encode_images_plan(recs, opts(S.ADAPTIVE_FAST))
    assert p["run_strategy"] == [S.SUB, S.ADAPTIVE_FAST, S.ADAPTIVE_FAST, S.ADAPTIVE_FAST, S.SUB]
    assert p["way_in"] == [True, False, False, True, True]
    # NO_RAYON: every AdaptiveFast is the sequential form
    p = png.encode_images_plan(recs, opts(S.ADAPTIVE_FAST, flags=png.NO_RAYON))
    assert p["way_in"] == [True, False, False, False, True]
    p = png.encode_images_plan(recs, opts(S.ADAPTIVE, flags=png.NO_RAYON))
    assert p["way_in"] == [True] * 5
    # reductions (presets 1 and 2) and quantisation: every image by itself, no filter launch
    for preset in (1, 2):
        p = png.encode_images_plan(recs, opts(preset=preset))
        assert p["way_in"] == [False] * 5 and p["filter_launches"] == 0 and p["sub_first"] == [0, 5]
    o = opts(S.PAETH)
    o.quantization = png.QuantizationOptions(png.QuantizationMode.FORCE, 16, False)
    p = png.encode_images_plan(recs, o)
    assert p["way_in"] == [False] * 5 and p["filter_launches"] == 0


def test_plan_sub_batches():
    shapes = [(10, 10, RGB), (20, 5, RGBA), (7, 7, GRAY), (30, 30, RGB), (3, 3, GA), (9, 9, RGB)]
    full = [h * (w * ct.bytes_per_pixel() + 1) for w, h, ct in shapes]
    assert full == [310, 405, 56, 2730, 21, 252]
    recs = back_to_back(shapes)
    try:
        jpeg.debug_configure("png_batch_bytes=800")  # 310 + 405 + 56 = 771 | 2730 alone, over the limit | 21 + 252
        p = png.encode_images_plan(recs, opts(S.PAETH))
        assert p["sub_first"] == [0, 3, 4, 6]
        assert p["filter_launches"] == 3 + 1 + 2  # (RGB, RGBA, Gray | RGB | GrayAlpha, RGB: a class each, by their bytes per pixel)
        jpeg.debug_configure("png_batch_bytes=1")  # every image a sub-batch of its own
        assert png.encode_images_plan(recs, opts(S.PAETH))["sub_first"] == [0, 1, 2, 3, 4, 5, 6]
        jpeg.debug_configure("png_batch_bytes=3774")  # exactly all six
        assert png.encode_images_plan(recs, opts(S.PAETH))["sub_first"] == [0, 6]
        jpeg.debug_configure("png_batch_bytes=3773")
        assert png.encode_images_plan(recs, opts(S.PAETH))["sub_first"] == [0, 5, 6]
    finally:
        jpeg.debug_configure(None)
    assert png.encode_images_plan(recs, opts(S.PAETH))["sub_first"] == [0, 6]
    # the chunk limit: every image has at least one chunk, a sub-batch at most 1024
    tiny = [(1, 1, GRAY, 16 * i) for i in range(2500)]
    p = png.encode_images_plan(tiny, opts(S.NONE))
    assert p["sub_first"] == [0, 1024, 2048, 2500] and p["filter_launches"] == 3
    # two chunks an image (200 x 150 RGB: 90,150 bytes): 512 a sub-batch
    two = [(200, 150, RGB, 0)] * 513
    assert png.encode_images_plan(two, opts(S.NONE))["sub_first"] == [0, 512, 513]
    # a one-chunk image behind 511 two-chunk ones still fits; a two-chunk one does not
    assert png.encode_images_plan([(200, 150, RGB, 0)] * 511 + [(1, 1, GRAY, 0), (1, 1, GRAY, 0), (1, 1, GRAY, 0)], opts(S.NONE))["sub_first"] == [0, 513, 514]


def test_plan_filter_launches_follow_the_classes():
    A = S.ADAPTIVE
    rgba = lambda w, at=0: (w, 2, RGBA, at)
    # one class: RGBA, aligned, rows in the registers of 256 threads — however many images
    assert png.encode_images_plan([rgba(3000), rgba(4096), rgba(2100)] * 20, opts(A))["filter_launches"] == 1
    # either side of 16 KiB, 32 KiB and the stage (12,276 x 4 = 49,104 bytes is the last row the stage holds)
    widths = [4096, 4097, 8192, 8193, 12276, 12277]
    per = [png.encode_images_plan([rgba(w)], opts(A))["filter_launches"] for w in widths]
    assert per == [1] * 6
    assert png.encode_images_plan([rgba(w) for w in widths], opts(A))["filter_launches"] == 4  # regs | regs512 | general staged | general direct
    assert png.encode_images_plan([rgba(w) for w in widths], opts(S.BIGRAMS))["filter_launches"] == 3  # bigrams regs | bigrams staged | direct
    assert png.encode_images_plan([rgba(w) for w in widths], opts(S.PAETH))["filter_launches"] == 2  # general staged | general direct
    # all four colour types, rows of a multiple of 4 bytes at aligned and unaligned places: 4 x 2 classes of one kernel form
    mixed = []
    for ct in (GRAY, GA, RGB, RGBA):
        mixed += [(100, 50, ct, 0), (100, 50, ct, 32), (100, 50, ct, 1001)]
    assert png.encode_images_plan(mixed, opts(A))["filter_launches"] == 8
    assert png.encode_images_plan(mixed, opts(A), alignment=3)["filter_launches"] == 8  # (1001 + 3 is aligned, 0 + 3 and 32 + 3 are not)
    assert png.encode_images_plan(mixed, opts(A), alignment=2)["filter_launches"] == 4  # nothing is aligned
    # a row length that is no multiple of 4 is never in the aligned class
    assert png.encode_images_plan([(33, 70, RGB, 0), (33, 70, RGB, 1)], opts(A))["filter_launches"] == 1
    # the area rule sends small images to the general form beside the register form of the large ones
    assert png.encode_images_plan([(64, 64, RGBA, 0), (65, 64, RGBA, 1 << 20)], opts(A))["filter_launches"] == 2
    # everything at once: 4 colour types x aligned or not x row lengths around the three edges, two sub-batches' worth of classes
    everything = [(w, 2, RGBA, at) for w in widths for at in (0, 1)] + mixed
    # RGBA: {regs, regs512, general staged, general direct} x {aligned, not} = 8, with the 100-wide RGBA in the regs classes;
    # Gray, GrayAlpha, RGB: regs x {aligned, not} = 6
    assert png.encode_images_plan(everything, opts(A))["filter_launches"] == 14
