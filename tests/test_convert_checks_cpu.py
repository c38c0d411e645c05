"""The colour-conversion entries (pixo_hip_convert*, pixo_amd/csrc/convert_api.cpp) without a GPU: the numpy model against
values worked out by hand, the ABI, every refusal of every entry with its status, class and exact message in the documented
order (all before anything is enqueued), the layout of both targets, and the plan — kinds, forms, tiles, launches and
sub-batches — against values worked out here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import convert_model as M
from pixo_amd import ColorType, _lib, convert, error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pixo_hip_convert_images_layout", "pixo_hip_convert_images_device", "pixo_hip_convert_images", "pixo_hip_convert_device", "pixo_hip_convert",
         "pixo_hip_debug_convert_images_plan")
GRAY, GRAY_ALPHA, RGB, RGBA = 0, 1, 2, 3
MAXD = 1 << 24
HELD = np.zeros(64, np.uint8)  # something non-null to point at: no refusal below reads it
COLOR_MESSAGE = "Invalid color type: %d. Expected 0 (Gray), 1 (GrayAlpha), 2 (Rgb), or 3 (Rgba)"
UNSUPPORTED = "Unsupported color type for this format"


# ---- the model, by hand ------------------------------------------------------------------------------------------------------
def test_model_against_values_derived_by_hand():
    def gray(*rgb):
        return M.convert(np.array(rgb, np.uint8), RGB, GRAY).tolist()
    # 77 + 150 + 29 = 256, so white is (256 * 255 + 128) >> 8 = 65408 >> 8 = 255 and black 128 >> 8 = 0.
    # red:   77 * 255 + 128 = 19763 = 77 * 256 + 51   -> 77  (the float weight 0.299 * 255 would truncate to 76; the reference's
    #        integer formula, src/bin/pixo.rs:489, rounds to nearest and gives 77 — that formula is what every entry is pinned to)
    # green: 150 * 255 + 128 = 38378 = 149 * 256 + 234 -> 149
    # blue:  29 * 255 + 128 = 7523 = 29 * 256 + 99     -> 29
    assert gray(255, 255, 255) == [255] and gray(0, 0, 0) == [0]
    assert gray(255, 0, 0) == [77] and gray(0, 255, 0) == [149] and gray(0, 0, 255) == [29]
    assert gray(1, 1, 1) == [1] and gray(254, 255, 255) == [255] and gray(0, 0, 4) == [0] and gray(0, 0, 5) == [1]  # 145 + 128 = 273 >> 8
    assert M.convert(np.array([255, 0, 0, 7, 0, 255, 0, 200], np.uint8), RGBA, GRAY).tolist() == [77, 149]  # (alpha ignored)
    assert M.convert(np.array([255, 128, 64, 255, 0, 100, 200, 128], np.uint8), RGBA, RGB).tolist() == [255, 128, 64, 0, 100, 200]
    assert M.convert(np.array([100, 255, 150, 128], np.uint8), GRAY_ALPHA, GRAY).tolist() == [100, 150]
    for ct in range(4):
        px = np.arange(12, dtype=np.uint8)
        assert M.convert(px, ct, ct).tolist() == px.tolist()
    for pair in [(GRAY, RGB), (GRAY, GRAY_ALPHA), (RGB, RGBA), (GRAY_ALPHA, RGB), (RGBA, GRAY_ALPHA), (RGB, GRAY_ALPHA), (GRAY, RGBA), (GRAY_ALPHA, RGBA)]:
        assert M.kind_of(*pair) is None
    assert [M.target_type(M.OPAQUE, ct) for ct in range(4)] == [GRAY, GRAY, RGB, RGB]
    assert [M.target_type(M.TO_GRAY, ct) for ct in range(4)] == [GRAY] * 4


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pixo_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"\buint32_t pixo_hip_debug_convert_tile_pixels\s*\(void\)", hdr) and hasattr(lib, "pixo_hip_debug_convert_tile_pixels")
    assert re.search(r"#define PIXO_CONVERT_OPAQUE 0\b", hdr) and re.search(r"#define PIXO_CONVERT_GRAY 1\b", hdr)
    assert (int(convert.Target.OPAQUE), int(convert.Target.GRAY)) == (0, 1)
    t = convert.tile_pixels()
    assert t % (16 * 256) == 0 and t > 0  # 16 pixels a lane x the workgroup size


def images_c(rows):
    arr = (_lib.PngImageC * max(len(rows), 1))()
    for i, (w, h, ct, at) in enumerate(rows):
        arr[i].width, arr[i].height, arr[i].color_type, arr[i].offset = w, h, ct, at
    return arr


def _call(entry, src, dst, batch=None, src_arr="own", dst_arr="own", d_src=True, d_dst=True, data_len=1 << 40, out=True, out_len=True, last=True):
    """One of the three images entries; `last` False: the plan's first out-pointer is null"""
    L = _lib.load()
    n = len(src) if batch is None else batch
    a = images_c(src) if src_arr == "own" else src_arr
    b = images_c(dst) if dst_arr == "own" else dst_arr
    p = HELD.ctypes.data
    if entry == "device":
        return L.pixo_hip_convert_images_device(p if d_src else None, a, p if d_dst else None, b, n, None)
    if entry == "host":
        o, ol = C.POINTER(C.c_uint8)(), C.c_size_t()
        return L.pixo_hip_convert_images(p if d_src else None, data_len, a, b, n, C.byref(o) if out else None, C.byref(ol) if out_len else None)
    sub, subs, la = (C.c_uint32 * (n + 2))(), C.c_uint32(), C.c_uint32()
    kind, form, tiles = (C.c_uint8 * max(n, 1))(), (C.c_uint8 * max(n, 1))(), (C.c_uint32 * max(n, 1))()
    return L.pixo_hip_debug_convert_images_plan(a, b, n, 0, 0, sub if last else None, C.byref(subs), kind, form, tiles, C.byref(la))


def _refused(rc, cls, message):
    with pytest.raises(cls) as e:
        _lib.check(rc)
    assert str(e.value) == message, str(e.value)


ENTRIES = ("device", "host", "plan")
OK_S, OK_D = (3, 2, RGBA, 0), (3, 2, RGB, 0)


@pytest.mark.parametrize("entry", ENTRIES)
def test_images_refusals_in_their_documented_order(entry):
    r = lambda *a, **k: _call(entry, *a, **k)  # noqa: E731
    C_ = error.CompressionError
    _refused(r([OK_S], [OK_D], src_arr=None, batch=0), C_, "Compression error: null argument 'src_images'")
    _refused(r([OK_S], [OK_D], dst_arr=None, batch=0), C_, "Compression error: null argument 'dst_images'")
    for n in (0, 65536):
        _refused(r([OK_S], [OK_D], batch=n), C_, "Compression error: batch must be 1..65535")
    # per image, in order: the sides (source, then destination), the colour types, the sizes, the pair, the offsets
    _refused(r([(0, 2, 9, 0)], [(0, 0, 9, 0)]), error.InvalidDimensions, "Invalid image dimensions: 0x2 (image 0)")
    _refused(r([(3, 2, 9, 0)], [(3, 0, 9, 0)]), error.InvalidDimensions, "Invalid image dimensions: 3x0 (image 0)")
    _refused(r([(MAXD + 1, 2, 9, 0)], [OK_D]), error.ImageTooLarge, "Image %dx2 exceeds maximum dimension %d (image 0)" % (MAXD + 1, MAXD))
    _refused(r([OK_S], [(3, MAXD + 1, 9, 0)]), error.ImageTooLarge, "Image 3x%d exceeds maximum dimension %d (image 0)" % (MAXD + 1, MAXD))
    _refused(r([(3, 2, 4, 0)], [(4, 2, 5, 0)]), error.InvalidColorArgument, COLOR_MESSAGE % 4 + " (image 0)")
    _refused(r([OK_S], [(4, 2, 5, 0)]), error.InvalidColorArgument, COLOR_MESSAGE % 5 + " (image 0)")
    _refused(r([(3, 2, GRAY, 0)], [(2, 3, RGB, 0)]), C_, "Compression error: sizes differ (image 0)")
    _refused(r([(3, 2, GRAY, 0)], [(3, 3, RGB, 0)]), C_, "Compression error: sizes differ (image 0)")
    for pair in [(GRAY, RGB), (GRAY, GRAY_ALPHA), (GRAY, RGBA), (GRAY_ALPHA, RGB), (GRAY_ALPHA, RGBA), (RGB, GRAY_ALPHA), (RGB, RGBA), (RGBA, GRAY_ALPHA)]:
        _refused(r([(3, 2, pair[0], 1 << 63)], [(3, 2, pair[1], 0)]), error.UnsupportedColorType, UNSUPPORTED + " (image 0)")
    _refused(r([(3, 2, RGBA, (1 << 62) - 23)], [(3, 2, RGB, 1 << 63)]), C_, "Compression error: batch input too large (image 0)")
    _refused(r([(3, 2, RGBA, (1 << 62) + 1)], [OK_D]), C_, "Compression error: batch input too large (image 0)")
    _refused(r([OK_S], [(3, 2, RGB, (1 << 62) - 17)]), C_, "Compression error: batch output too large (image 0)")
    fits = r([(3, 2, RGBA, (1 << 62) - 24)], [(3, 2, RGB, (1 << 62) - 18)], d_src=False)  # both just fit: the next check answers
    assert (fits == 0) == (entry == "plan") and (entry == "plan" or "null argument 'd" in _lib.load().pixo_hip_last_error().decode())
    # a later image fails differently: the first failing image answers
    _refused(r([OK_S, (3, 2, GRAY, 0), (0, 1, RGB, 0)], [OK_D, (3, 2, RGB, 0), (0, 1, RGB, 0)]), error.UnsupportedColorType, UNSUPPORTED + " (image 1)")
    _refused(r([OK_S, OK_S, (0, 1, RGB, 0)], [OK_D, OK_D, (3, 2, 7, 0)]), error.InvalidDimensions, "Invalid image dimensions: 0x1 (image 2)")
    # behind all per-image checks: the blocks / the out-pointers
    if entry == "device":
        _refused(r([OK_S], [OK_D], d_src=False, d_dst=False), C_, "Compression error: null argument 'd_src'")
        _refused(r([OK_S], [OK_D], d_dst=False), C_, "Compression error: null argument 'd_dst'")
        _refused(r([OK_S, (0, 1, RGB, 0)], [OK_D, OK_D], d_src=False), error.InvalidDimensions, "Invalid image dimensions: 0x1 (image 1)")
    elif entry == "host":
        _refused(r([OK_S], [OK_D], d_src=False, out=False), C_, "Compression error: null argument 'data'")
        _refused(r([OK_S], [OK_D], out=False, out_len=False), C_, "Compression error: null argument 'out'")
        _refused(r([OK_S], [OK_D], out_len=False, data_len=0), C_, "Compression error: null argument 'out_len'")
        _refused(r([OK_S, (2, 2, GRAY, 100)], [OK_D, (2, 2, GRAY, 32)], data_len=103), error.InvalidDataLength,
                 "Invalid pixel data length: expected 104 bytes, got 103")
    else:
        _refused(r([OK_S], [OK_D], last=False), C_, "Compression error: null argument 'sub_first'")


def test_layout_refusals_in_their_documented_order():
    L = _lib.load()
    out, total = (_lib.PngImageC * 4)(), C.c_size_t(77)

    def r(rows, target=0, batch=None, src="own", dst=out, tot=True):
        return L.pixo_hip_convert_images_layout(images_c(rows) if src == "own" else src, len(rows) if batch is None else batch, target, dst,
                                                C.byref(total) if tot else None)
    C_ = error.CompressionError
    _refused(r([OK_S], src=None, dst=None, batch=0), C_, "Compression error: null argument 'src_images'")
    _refused(r([OK_S], dst=None, tot=False, batch=0), C_, "Compression error: null argument 'dst_images'")
    _refused(r([OK_S], tot=False, batch=0), C_, "Compression error: null argument 'total'")
    for n in (0, 65536):
        _refused(r([OK_S], batch=n, target=9), C_, "Compression error: batch must be 1..65535")
    _refused(r([(0, 0, 9, 0)], target=2), C_, "Compression error: unknown convert target 2")
    _refused(r([OK_S, (0, 5, 9, 0)]), error.InvalidDimensions, "Invalid image dimensions: 0x5 (image 1)")
    _refused(r([OK_S, (5, MAXD + 1, 9, 0)]), error.ImageTooLarge, "Image 5x%d exceeds maximum dimension %d (image 1)" % (MAXD + 1, MAXD))
    _refused(r([OK_S, (5, 5, 4, 0), (0, 0, 0, 0)]), error.InvalidColorArgument, COLOR_MESSAGE % 4 + " (image 1)")
    assert r([(MAXD, MAXD, RGBA, 0)] * 4) == 0  # (3 x 2^48 bytes each)
    many = images_c([(MAXD, MAXD, RGB, 0)] * 65535)
    dst = (_lib.PngImageC * 65535)()
    _refused(L.pixo_hip_convert_images_layout(many, 65535, 0, dst, C.byref(total)), C_, "Compression error: batch output too large")
    assert all(d.width == 0 for d in dst)  # nothing is written before every check has passed


def test_single_entry_refusals_in_their_documented_order():
    L = _lib.load()
    p = HELD.ctypes.data
    o, ol = C.POINTER(C.c_uint8)(), C.c_size_t()

    def dev(w, h, s, d, src=p, dst=p):
        return L.pixo_hip_convert_device(src, w, h, s, d, dst, None)

    def host(w, h, s, d, data=p, n=0, out=C.byref(o), out_len=C.byref(ol)):
        return L.pixo_hip_convert(data, n, w, h, s, d, out, out_len)
    for f in (dev, host):
        _refused(f(0, 3, 9, 9), error.InvalidDimensions, "Invalid image dimensions: 0x3")
        _refused(f(3, 0, 9, 9), error.InvalidDimensions, "Invalid image dimensions: 3x0")
        _refused(f(MAXD + 1, 3, 9, 9), error.ImageTooLarge, "Image %dx3 exceeds maximum dimension %d" % (MAXD + 1, MAXD))
        _refused(f(3, 3, 4, 9), error.InvalidColorArgument, COLOR_MESSAGE % 4)
        _refused(f(3, 3, RGB, 9), error.InvalidColorArgument, COLOR_MESSAGE % 9)
        _refused(f(3, 3, GRAY, RGB), error.UnsupportedColorType, UNSUPPORTED)
        _refused(f(3, 3, RGB, RGBA), error.UnsupportedColorType, UNSUPPORTED)
    _refused(dev(3, 3, RGBA, RGB, src=None, dst=None), error.CompressionError, "Compression error: null argument 'd_src'")
    _refused(dev(3, 3, RGBA, RGB, dst=None), error.CompressionError, "Compression error: null argument 'd_dst'")
    _refused(host(3, 3, RGBA, RGB, out=None, out_len=None), error.CompressionError, "Compression error: null argument 'out'")
    _refused(host(3, 3, RGBA, RGB, out_len=None), error.CompressionError, "Compression error: null argument 'out_len'")
    _refused(host(3, 3, RGBA, RGB, n=35, data=None), error.InvalidDataLength, "Invalid pixel data length: expected 36 bytes, got 35")
    _refused(host(3, 3, RGBA, RGB, n=36, data=None), error.CompressionError, "Compression error: null argument 'data'")
    # the wrappers of the front end's names check what they can without a device
    with pytest.raises(ValueError):
        convert.rgba_to_rgb(bytes(7))
    assert convert.rgba_to_rgb(b"") == b"" and convert.to_grayscale(b"", ColorType.Rgb) == b""


# ---- the layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", (M.OPAQUE, M.TO_GRAY))
def test_layout_of_both_targets_over_all_colour_types(target):
    rows = [(5, 3, GRAY, 999), (5, 3, GRAY_ALPHA, 7), (5, 3, RGB, 0), (5, 3, RGBA, 1 << 40), (16, 1, RGBA, 3), (1, 1, GRAY_ALPHA, 0), (7, 7, RGB, 1)]
    got, total = convert.layout_images(rows, target)
    at, want = 0, []
    for w, h, ct, _ in rows:
        d = M.target_type(target, ct)
        want.append((w, h, d, at))
        end = at + w * h * (d + 1)
        at = (end + 15) // 16 * 16
    assert [(w, h, int(ct), o) for w, h, ct, o in got] == want and total == end
    # ... by hand, for OPAQUE: 15, 15, 45, 45, 48, 1, 147 bytes at 0, 16, 32, 80, 128, 176, 192; total 339
    if target == M.OPAQUE:
        assert [o for _, _, _, o in got] == [0, 16, 32, 80, 128, 176, 192] and total == 339
        assert [int(ct) for _, _, ct, _ in got] == [GRAY, GRAY, RGB, RGB, RGB, GRAY, RGB]
    else:
        assert [o for _, _, _, o in got] == [0, 16, 32, 48, 64, 80, 96] and total == 96 + 49
    # `reserved` zeroed, and in place
    L = _lib.load()
    arr = images_c(rows)
    for im in arr:
        for k in range(7):
            im.reserved[k] = 0xEE
    n = C.c_size_t()
    _lib.check(L.pixo_hip_convert_images_layout(arr, len(rows), target, arr, C.byref(n)))
    assert [(im.width, im.height, im.color_type, im.offset) for im in arr] == want and n.value == total
    assert all(b == 0 for im in arr for b in im.reserved)


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def _dst(rows, cts):
    return [(w, h, ct, o) for (w, h, _, o), ct in zip(rows, cts)]


def test_plan_launch_counts_follow_the_classes_present():
    T = convert.tile_pixels()
    same = [(40, 30, RGB, 16 * 300 * i) for i in range(5)]
    p = convert.convert_images_plan(same, same)
    assert p == dict(sub_first=[0, 5], kind=[0] * 5, form=[0] * 5, tiles=[1] * 5, launches=1)
    # all five kinds x both forms: the odd images start one byte behind a multiple of 16
    pairs = [(RGB, RGB), (GRAY_ALPHA, GRAY), (RGBA, RGB), (RGB, GRAY), (RGBA, GRAY)]
    src = [(9, 9, s, 1024 * i + (i % 2)) for i, (s, _) in enumerate(pairs * 2)]
    dst = [(9, 9, d, 1024 * i) for i, (_, d) in enumerate(pairs * 2)]
    src[5:] = [(9, 9, s, 1024 * (5 + i) + (0 if i % 2 else 1)) for i, (s, _) in enumerate(pairs)]  # each kind once aligned, once not
    p = convert.convert_images_plan(src, dst)
    assert p["kind"] == [0, 1, 2, 3, 4] * 2 and p["form"] == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1] and p["launches"] == 10 and p["sub_first"] == [0, 10]
    # the copy of any bytes per pixel is one class
    mix = [(9, 9, ct, 1024 * ct) for ct in range(4)]
    assert convert.convert_images_plan(mix, mix)["launches"] == 1
    # tiles: one per T pixels
    sizes = [(1, 1), (T - 1, 1), (T, 1), (T + 1, 1), (64, 65), (T, 5), (T, 5 * 13)]
    rows = [(w, h, RGBA, 0) for w, h in sizes]
    assert convert.convert_images_plan(rows, _dst(rows, [GRAY] * len(rows)))["tiles"] == [1, 1, 1, 2, 2, 5, 65]
    assert (64 * 65 + T - 1) // T == 2 or T != 4096


def test_plan_form_per_address_residues():
    rows_s, rows_d = [(17, 1, RGBA, 0), (17, 1, RGBA, 80), (17, 1, RGBA, 161)], [(17, 1, RGB, 0), (17, 1, RGB, 65), (17, 1, RGB, 128)]
    for sa in range(16):
        for da in range(16):
            p = convert.convert_images_plan(rows_s, rows_d, sa, da)
            want = [int((sa + so) % 16 != 0 or (da + do) % 16 != 0) for (_, _, _, so), (_, _, _, do) in zip(rows_s, rows_d)]
            assert p["form"] == want, (sa, da)
    # ... in words: an odd block makes an image aligned whose offset makes up for it
    assert convert.convert_images_plan(rows_s, rows_d, 15, 0)["form"] == [1, 1, 0]


def test_plan_sub_batches_under_the_debug_switch():
    T = convert.tile_pixels()
    L = _lib.load()
    five = [(T, 5, RGBA, 0)] * 6
    dst = _dst(five, [RGB] * 6)
    try:
        L.pixo_hip_debug_configure(b"convert_images_tiles=2")
        # an image has at most 2 tiles, a launch at most 4: two images of a class per sub-batch
        p = convert.convert_images_plan(five, dst)
        assert p["tiles"] == [2] * 6 and p["sub_first"] == [0, 2, 4, 6] and p["launches"] == 3
        # classes fill up separately: the gray images do not count against the RGB launch
        mixed = [(T, 5, RGBA, 0), (T, 5, GRAY, 0), (T, 5, RGBA, 0), (T, 5, GRAY, 0), (10, 1, RGBA, 0), (T, 5, RGBA, 0)]
        p = convert.convert_images_plan(mixed, _dst(mixed, [RGB, GRAY, RGB, GRAY, RGB, RGB]))
        assert p["tiles"] == [2, 2, 2, 2, 1, 2] and p["sub_first"] == [0, 4, 6] and p["launches"] == 3
        L.pixo_hip_debug_configure(b"convert_images_tiles=1")
        p = convert.convert_images_plan(five, dst)
        assert p["tiles"] == [1] * 6 and p["sub_first"] == [0, 2, 4, 6]
    finally:
        L.pixo_hip_debug_configure(None)
    assert convert.convert_images_plan(five, dst) == dict(sub_first=[0, 6], kind=[2] * 6, form=[0] * 6, tiles=[5] * 6, launches=1)
    # the cap of an image's tiles, and the 2^31 - 1 tiles of a launch: 65536 tiles an image, so 32767 such images fit a launch
    huge = [(MAXD, 1 << 10, GRAY, 0)] * 40000  # 2^34 pixels each
    p = convert.convert_images_plan(huge, huge)
    assert set(p["tiles"]) == {65536} and p["sub_first"] == [0, 32767, 40000] and p["launches"] == 2


def test_plan_of_the_largest_batch():
    rows = [(1, 1, i % 4, 16 * i) for i in range(65535)]
    dst, total = convert.layout_images(rows, convert.Target.GRAY)
    assert total == 16 * 65534 + 1
    p = convert.convert_images_plan(rows, dst)
    assert p["sub_first"] == [0, 65535] and p["tiles"] == [1] * 65535 and p["launches"] == 4
    assert p["kind"][:4] == [M.K_COPY, M.K_GA_G, M.K_RGB_G, M.K_RGBA_G]
