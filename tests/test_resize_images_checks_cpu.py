"""The resize images entries (pixo_hip_resize_images*, pixo_amd/csrc/resize_api.cpp) without a GPU: the ABI, every refusal
with its status, class and exact message in the documented order (all before anything is enqueued), the plan — sub-batches,
offsets into the intermediate, LDS staging per image, shared axis tables, tiles and launches per pass — against values worked
out here, and the fitted sizes against a restatement of the reference front end's calculateResizeDimensions."""
import ctypes as C
import math
import os
import random
import re

import numpy as np
import pytest

import resize_cases as RC
import resize_reach_cases as RR
from pixo_amd import ColorType, _lib, decode, error, jpeg, png, resize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pixo_hip_resize_images_fit", "pixo_hip_resize_images_device", "pixo_hip_resize_images", "pixo_hip_debug_resize_images_plan")
NEAREST, BILINEAR, LANCZOS3 = 0, 1, 2
GRAY, GRAY_ALPHA, RGB, RGBA = 0, 1, 2, 3
MAXD = 1 << 24
HELD = np.zeros(64, np.uint8)  # something non-null to point at: no refusal below reads it
COLOR_MESSAGE = "Invalid color type: %d. Expected 0 (Gray), 1 (GrayAlpha), 2 (Rgb), or 3 (Rgba)"


def test_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pixo_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define PIXO_RESIZE_FIT_NO_ENLARGE 1u", hdr) and resize.FIT_NO_ENLARGE == 1


def test_route_bit_is_the_next_free_one():
    routes = open(os.path.join(ROOT, "pixo_amd", "csrc", "routes.hpp")).read()
    assert re.search(r"\bRESIZE_IMAGES = 1ull << 47,", routes)
    assert resize.ROUTES["RESIZE_IMAGES"] == 47 and resize.ROUTE_RESIZE_IMAGES == 1 << 47
    others = set(png.ROUTES.values()) | set(png.IMAGES_ROUTES.values()) | set(jpeg.ROUTES.values()) | set(decode.ROUTES.values()) | \
        set(decode.INFLATE_ROUTES.values()) | {v for k, v in resize.ROUTES.items() if k != "RESIZE_IMAGES"}
    assert 47 not in others and max(others) == 46
    assert [int(b) for b in re.findall(r"= 1ull << (\d+),", routes)] == list(range(48))


def images_c(rows):
    """rows of (width, height, colour type, offset)"""
    arr = (_lib.PngImageC * max(len(rows), 1))()
    for i, (w, h, ct, at) in enumerate(rows):
        arr[i].width, arr[i].height, arr[i].color_type, arr[i].offset = w, h, ct, at
    return arr


def _call(entry, src, dst, algo=LANCZOS3, batch=None, src_arr="own", dst_arr="own", d_src=True, d_dst=True, data_len=1 << 40, out=True, out_len=True,
          last=True):
    """One of the three entries; `last` False: the plan's first out-pointer is null"""
    L = _lib.load()
    n = len(src) if batch is None else batch
    a = images_c(src) if src_arr == "own" else src_arr
    b = images_c(dst) if dst_arr == "own" else dst_arr
    held = HELD.ctypes.data
    if entry == "device":
        return L.pixo_hip_resize_images_device(held if d_src else None, a, held if d_dst else None, b, n, algo, None)
    if entry == "host":
        o, o_len = C.POINTER(C.c_uint8)(), C.c_size_t()
        return L.pixo_hip_resize_images(held if d_src else None, data_len, a, b, n, algo, C.byref(o) if out else None, C.byref(o_len) if out_len else None)
    sub_first, mid_at, use_lds = (C.c_uint32 * (n + 1))(), (C.c_uint64 * max(n, 1))(), (C.c_uint8 * max(n, 1))()
    t1, t2 = (C.c_uint32 * max(n, 1))(), (C.c_uint32 * max(n, 1))()
    subs, tables, l1, l2 = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    return L.pixo_hip_debug_resize_images_plan(a, b, n, algo, sub_first if last else None, C.byref(subs), mid_at, use_lds, t1, t2, C.byref(tables),
                                               C.byref(l1), C.byref(l2))


def _refused(entry, status, cls, message, *args, **kw):
    rc = _call(entry, *args, **kw)
    got = _lib.load().pixo_hip_last_error().decode()
    assert (rc, got) == (status, message), (entry, rc, got)
    assert type(error.from_status(rc, got)) is cls


ENTRIES = ("device", "host", "plan")
S0, S1 = (37, 23, RGB, 0), (64, 41, RGBA, 2560)
D0, D1 = (17, 13, RGB, 0), (5, 9, RGBA, 672)

# (sources, destinations, algorithm) -> status, class, the single entry's message, the image it is reported for
REFUSALS = [
    (([S0, S1, (0, 5, RGB, 0)], [D0, D1, D0], LANCZOS3), -1, error.InvalidDimensions, "Invalid image dimensions: 0x5", 2),
    (([S0, (5, 0, RGB, 0)], [D0, D0], NEAREST), -1, error.InvalidDimensions, "Invalid image dimensions: 5x0", 1),
    (([S0, S1], [(0, 13, RGB, 0), D1], BILINEAR), -1, error.InvalidDimensions, "Invalid image dimensions: 0x13", 0),
    (([S0, S1], [D0, (5, 0, RGBA, 0)], LANCZOS3), -1, error.InvalidDimensions, "Invalid image dimensions: 5x0", 1),
    (([S0, (MAXD + 1, 2, GRAY, 0)], [D0, (17, 13, GRAY, 0)], NEAREST), -4, error.ImageTooLarge, "Image %dx13 exceeds maximum dimension %d" % (MAXD + 1, MAXD), 1),
    (([S0], [(17, MAXD + 1, RGB, 0)], NEAREST), -4, error.ImageTooLarge, "Image 37x%d exceeds maximum dimension %d" % (MAXD + 1, MAXD), 0),
    (([S0, (3, 3, 4, 0)], [D0, (3, 3, 4, 0)], LANCZOS3), -8, error.InvalidColorArgument, COLOR_MESSAGE % 4, 1),
    (([S0, S1], [D0, D1], 3), -8, error.InvalidColorArgument, "Invalid resize algorithm: 3. Expected 0 (Nearest), 1 (Bilinear), or 2 (Lanczos3)", 0),
    # the single entry's order within one image: source size, destination size, too large, colour type, algorithm
    (([(0, 0, 9, 0)], [(0, 0, 8, 0)], 9), -1, error.InvalidDimensions, "Invalid image dimensions: 0x0", 0),
    (([(1, 1, 9, 0)], [(MAXD + 1, 1, 8, 0)], 9), -4, error.ImageTooLarge, "Image %dx1 exceeds maximum dimension %d" % (MAXD + 1, MAXD), 0),
    (([(1, 1, 9, 0)], [(1, 1, 8, 0)], 9), -8, error.InvalidColorArgument, COLOR_MESSAGE % 9, 0),
]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("r", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_an_image_is_refused_with_the_single_entrys_status_and_message(entry, r):
    args, status, cls, message, image = r
    _refused(entry, status, cls, "%s (image %d)" % (message, image), *args)


def test_the_message_is_the_single_entrys():
    """... which is pinned to the reference by tests/golden/resize_cases.json: same call through pixo_hip_resize_device"""
    L = _lib.load()
    for (src, dst, algo), status, _, message, image in REFUSALS:
        o = _lib.ResizeOptionsC(src[image][0], src[image][1], dst[image][0], dst[image][1], src[image][2], algo)
        assert L.pixo_hip_resize_device(HELD.ctypes.data, C.byref(o), HELD.ctypes.data, None) == status
        assert L.pixo_hip_last_error().decode() == message


@pytest.mark.parametrize("entry", ENTRIES)
def test_colour_types_and_offsets(entry):
    differ = "Compression error: colour types differ (image 1)"
    _refused(entry, -6, error.CompressionError, differ, [S0, S1], [D0, (5, 9, RGB, 672)])
    _refused(entry, -6, error.CompressionError, differ, [S0, S1], [D0, (5, 9, 4, 672)])  # (a code that is no colour type differs too)
    # the single entry's checks on an image come before its colour types are compared, those before its offsets
    _refused(entry, -1, error.InvalidDimensions, "Invalid image dimensions: 5x0 (image 1)", [S0, S1], [D0, (5, 0, RGB, 1 << 63)])
    _refused(entry, -6, error.CompressionError, differ, [S0, (64, 41, RGBA, 1 << 63)], [D0, (5, 9, RGB, 1 << 63)])
    most = 1 << 62
    big_in, big_out = "Compression error: batch input too large (image %d)", "Compression error: batch output too large (image %d)"
    _refused(entry, -6, error.CompressionError, big_in % 1, [S0, (64, 41, RGBA, most - 64 * 41 * 4 + 1)], [D0, D1])
    _refused(entry, -6, error.CompressionError, big_in % 0, [(37, 23, RGB, most + 1), S1], [D0, D1])
    _refused(entry, -6, error.CompressionError, big_in % 0, [(37, 23, RGB, (1 << 64) - 1), S1], [D0, D1])
    _refused(entry, -6, error.CompressionError, big_out % 1, [S0, S1], [D0, (5, 9, RGBA, most - 5 * 9 * 4 + 1)])
    _refused(entry, -6, error.CompressionError, big_in % 0, [(37, 23, RGB, most), S1], [(17, 13, RGB, most), D1])  # the source's side first
    # an image that ends at 2^62 exactly passes these checks: the next refusal answers
    last = {"device": "d_dst", "host": "out", "plan": "sub_first"}[entry]
    _refused(entry, -6, error.CompressionError, "Compression error: null argument '%s'" % last,
             [S0, (64, 41, RGBA, most - 64 * 41 * 4)], [D0, (5, 9, RGBA, most - 5 * 9 * 4)], d_dst=False, out=False, last=False)


@pytest.mark.parametrize("entry", ENTRIES)
def test_order_of_refusals(entry):
    bad = (0, 7, RGB, 0)
    null = "Compression error: null argument '%s'"
    batch = "Compression error: batch must be 1..65535"
    # src_images, then dst_images, then batch, then the images, then the entry's pointers
    _refused(entry, -6, error.CompressionError, null % "src_images", [bad], [bad], batch=0, src_arr=None, dst_arr=None, d_src=False, d_dst=False)
    _refused(entry, -6, error.CompressionError, null % "dst_images", [bad], [bad], batch=0, dst_arr=None, d_src=False, d_dst=False)
    _refused(entry, -6, error.CompressionError, batch, [bad], [bad], batch=0, d_src=False, d_dst=False)
    big = (_lib.PngImageC * 65536)()  # (zeroed: were the batch accepted, image 0 would be refused instead)
    _refused(entry, -6, error.CompressionError, batch, [], [], batch=65536, src_arr=big, dst_arr=big)
    _refused(entry, -1, error.InvalidDimensions, "Invalid image dimensions: 0x0 (image 0)", [], [], batch=65535, src_arr=big, dst_arr=big)
    _refused(entry, -1, error.InvalidDimensions, "Invalid image dimensions: 0x7 (image 2)", [S0, S1, bad, S0], [D0, D1, D0, D0], d_src=False, d_dst=False,
             out=False, last=False)
    # the first failing image answers, whatever its failure: image 0's colour types before image 1's size
    _refused(entry, -6, error.CompressionError, "Compression error: colour types differ (image 0)", [S0, bad], [(17, 13, GRAY, 0), D0])
    _refused(entry, -4, error.ImageTooLarge, "Image %dx13 exceeds maximum dimension %d (image 0)" % (MAXD + 1, MAXD),
             [(MAXD + 1, 1, RGB, 0), S1, bad], [D0, D1, D0])
    if entry == "device":
        _refused(entry, -6, error.CompressionError, null % "d_src", [S0, S1], [D0, D1], d_src=False, d_dst=False)
        _refused(entry, -6, error.CompressionError, null % "d_dst", [S0, S1], [D0, D1], d_dst=False)
    if entry == "host":
        _refused(entry, -6, error.CompressionError, null % "data", [S0, S1], [D0, D1], d_src=False, out=False, data_len=0)
        _refused(entry, -6, error.CompressionError, null % "out", [S0, S1], [D0, D1], out=False, out_len=False, data_len=0)
        _refused(entry, -6, error.CompressionError, null % "out_len", [S0, S1], [D0, D1], out_len=False, data_len=0)
        end = 2560 + 64 * 41 * 4  # the furthest source's end, not the last's
        for srcs in ([S0, S1], [S1, S0]):
            _refused(entry, -2, error.InvalidDataLength, "Invalid pixel data length: expected %d bytes, got %d" % (end, end - 1), srcs, [D0, D1][::1 if srcs[0] == S0 else -1],
                     data_len=end - 1)
    if entry == "plan":
        _refused(entry, -6, error.CompressionError, null % "sub_first", [S0, S1], [D0, D1], last=False)


def test_the_length_message_is_worded_as_png_encode_images_words_it():
    L = _lib.load()
    o = png.PngOptions.builder(1, 1).build().to_c()
    files, lens = (C.POINTER(C.c_uint8) * 1)(), (C.c_size_t * 1)()
    assert L.pixo_hip_png_encode_images(HELD.ctypes.data, 10, images_c([(3, 3, RGB, 16)]), 1, C.byref(o), None, files, lens) == -2
    theirs = L.pixo_hip_last_error().decode()
    _call("host", [(3, 3, RGB, 16)], [(2, 2, RGB, 0)], data_len=10)
    assert L.pixo_hip_last_error().decode() == theirs == "Invalid pixel data length: expected 43 bytes, got 10"


def test_python_raises_the_errors_class_and_checks_sizes():
    with pytest.raises(error.InvalidDimensions, match=r"^Invalid image dimensions: 0x5 \(image 1\)$"):
        resize.resize_images_device(HELD.ctypes.data, [(3, 3, RGB, 0), (0, 5, RGB, 32)], HELD.ctypes.data, [(2, 2, RGB, 0), (2, 2, RGB, 16)], LANCZOS3)
    with pytest.raises(error.CompressionError, match=r"colour types differ \(image 0\)$"):
        resize.resize_images(np.zeros(27, np.uint8), [(3, 3, RGB, 0)], [(2, 2, RGBA, 0)], BILINEAR)
    with pytest.raises(error.InvalidDataLength, match="expected 27 bytes, got 26"):
        resize.resize_images(bytes(26), [(3, 3, RGB, 0)], [(2, 2, RGB, 0)], BILINEAR)
    with pytest.raises(error.CompressionError, match="batch must be 1..65535"):
        resize.resize_images_plan([], [], NEAREST)
    with pytest.raises(ValueError, match="2 sources, 1 destinations"):
        resize.resize_images_plan([(3, 3, RGB, 0), (3, 3, RGB, 32)], [(2, 2, RGB, 0)], NEAREST)
    torch = pytest.importorskip("torch")
    block, out = torch.zeros(59, dtype=torch.uint8), torch.zeros(28, dtype=torch.uint8)
    with pytest.raises(ValueError, match="the sources end at byte 59, the tensor holds 58"):
        resize.resize_images_device(block[:58], [(3, 3, RGB, 0), (3, 3, RGB, 32)], out, [(2, 2, RGB, 0), (2, 2, RGB, 16)], NEAREST)
    with pytest.raises(ValueError, match="the destinations end at byte 28, the tensor holds 27"):
        resize.resize_images_device(block, [(3, 3, RGB, 0), (3, 3, RGB, 32)], out[:27], [(2, 2, RGB, 0), (2, 2, RGB, 16)], NEAREST)


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def stride(dw, bpp):
    return (dw * bpp + 15) // 16 * 16


def expected_lds(sw, dw, bpp):
    return RR.max_span(*RR.taps(sw, dw)) * bpp + 8 <= RR.SEG_BYTES


def ceil_div(a, b):
    return -(-a // b)


def tiles(kind, sh, dw, dh, bpp, cap=65535):
    """A point tile is 256 columns x 4 rows, a horizontal one 64 columns x 4 SOURCE rows, a vertical one 1024 bytes x 1 row;
    an image has at most `cap` rows of tiles"""
    if kind == "point":
        return ceil_div(dw, 256) * min(ceil_div(dh, 4), cap)
    if kind == "h":
        return ceil_div(dw, 64) * min(ceil_div(sh, 4), cap)
    return ceil_div(dw * bpp, 1024) * min(dh, cap)


def expected_plan(srcs, dsts, algo, limit=256 << 20, cap=65535):
    """Greedy in order: an image joins the sub-batch while the intermediates stay within `limit`; every sub-batch holds one.
    (No launch of the cases here comes near 2^31 tiles.)"""
    lanczos = algo == LANCZOS3
    sub_first, mid_at, held, first, second, l1, l2 = [0], [], 0, set(), False, 0, 0
    for i, ((sw, sh, ct, _), (dw, dh, _, _)) in enumerate(zip(srcs, dsts)):
        rows = stride(dw, ct + 1) * sh if lanczos else 0
        if i > sub_first[-1] and held + rows > limit:
            sub_first.append(i)
            held, first, second = 0, set(), False
        l1 += ct not in first
        l2 += lanczos and not second
        first.add(ct)
        second = True
        mid_at.append(held)
        held += rows
    return dict(sub_first=sub_first + [len(srcs)], mid_at=mid_at,
                use_lds=[lanczos and expected_lds(s[0], d[0], s[2] + 1) for s, d in zip(srcs, dsts)],
                tiles_first=[tiles("h" if lanczos else "point", s[1], d[0], d[1], s[2] + 1, cap) for s, d in zip(srcs, dsts)],
                tiles_second=[tiles("v", s[1], d[0], d[1], s[2] + 1, cap) if lanczos else 0 for s, d in zip(srcs, dsts)],
                axis_tables=len({(s[0], d[0]) for s, d in zip(srcs, dsts)}) + len({(s[1], d[1]) for s, d in zip(srcs, dsts)}) if lanczos else 0,
                launches_first=l1, launches_second=l2)


SRC_SIZES = [(37, 23), (64, 41), (1, 1), (5, 300), (300, 5), (64, 41), (129, 7), (2200, 2)]
DST_SIZES = [(17, 13), (64, 41), (1, 1), (3, 3), (257, 5), (65, 9), (300, 6), (64, 2)]


def ragged(rotation=0, src_sizes=SRC_SIZES, dst_sizes=DST_SIZES):
    srcs = [(w, h, (i + rotation) % 4, 0) for i, (w, h) in enumerate(src_sizes)]
    dsts = [(w, h, (i + rotation) % 4, 0) for i, (w, h) in enumerate(dst_sizes)]
    return srcs, dsts


@pytest.mark.parametrize("rotation", range(4))
def test_plan_of_the_ragged_set(rotation):
    srcs, dsts = ragged(rotation)
    for algo in (NEAREST, BILINEAR, LANCZOS3):
        p = resize.resize_images_plan(srcs, dsts, algo)
        assert p == expected_plan(srcs, dsts, algo), algo
        assert p["launches_first"] == 4 and p["launches_second"] == (1 if algo == LANCZOS3 else 0)
        assert p["sub_first"] == [0, 8]
    p = resize.resize_images_plan(srcs, dsts, LANCZOS3)
    # (64, 41) -> (64, 41) and (64, 41) -> (65, 9) share nothing; no pair repeats: 8 + 8 tables
    assert p["axis_tables"] == 16
    # what the set is there for: two point tiles in x (257 columns), two horizontal tiles (65), two vertical tiles (1200 bytes at 4)
    q = resize.resize_images_plan(srcs, dsts, BILINEAR)
    assert q["tiles_first"][4] == 2 * 2 and p["tiles_first"][5] == 2 * 11
    assert p["tiles_second"][6] == (2 if (6 + rotation) % 4 == 3 else 1) * 6
    # the last source's 64 columns span all its 2200 pixels: 2200 * bpp + 8 bytes fit the 8192-byte segment at 1, 2 and 3 bytes a
    # pixel (6608 at 3) and not at 4 (8808): over the four rotations the image is staged three times and direct once, beside
    # staged images in the same launch
    assert RR.max_span(*RR.taps(2200, 64)) == 2200
    assert p["use_lds"][7] == ((7 + rotation) % 4 < 3) and all(p["use_lds"][:7])
    assert all(at % 16 == 0 for at in p["mid_at"])
    ends = [at + stride(d[0], s[2] + 1) * s[1] for at, s, d in zip(p["mid_at"], srcs, dsts)]
    assert p["mid_at"][0] == 0 and p["mid_at"][1:] == ends[:-1]  # every image's own stride, image after image


def test_plan_a_repeated_pair_is_shared():
    srcs = [(64, 41, RGB, 0), (64, 41, GRAY, 0), (64, 30, RGB, 0), (50, 41, RGB, 0), (64, 41, RGB, 0)]
    dsts = [(17, 13, RGB, 0), (17, 13, GRAY, 0), (17, 13, RGB, 0), (17, 13, RGB, 0), (17, 12, RGB, 0)]
    p = resize.resize_images_plan(srcs, dsts, LANCZOS3)
    # horizontal pairs: 64->17, 50->17; vertical pairs: 41->13, 30->13, 41->12 (the pixel size is no part of a table)
    assert p["axis_tables"] == 2 + 3 and p == expected_plan(srcs, dsts, LANCZOS3)
    # a (source, destination) pair met on the other axis is another table
    assert resize.resize_images_plan([(5, 9, GRAY, 0), (9, 5, GRAY, 0)], [(3, 4, GRAY, 0), (4, 3, GRAY, 0)], LANCZOS3)["axis_tables"] == 4
    assert resize.resize_images_plan([(5, 5, GRAY, 0)] * 3, [(3, 3, GRAY, 0)] * 3, LANCZOS3)["axis_tables"] == 2
    # one source size to two destination sizes: two tables per axis
    assert resize.resize_images_plan([(5, 5, GRAY, 0)] * 2, [(3, 3, GRAY, 0), (4, 4, GRAY, 0)], LANCZOS3)["axis_tables"] == 4


def test_plan_launches_follow_the_pixel_sizes_present():
    for cts, want in (([RGB] * 5, 1), ([RGB, RGBA, RGB, RGBA], 2), ([GRAY, RGBA, GRAY_ALPHA], 3), ([RGBA, RGB, GRAY_ALPHA, GRAY, RGB], 4)):
        srcs = [(20 + i, 10 + i, ct, 0) for i, ct in enumerate(cts)]
        dsts = [(7 + i, 5, ct, 0) for i, ct in enumerate(cts)]
        for algo in (NEAREST, BILINEAR, LANCZOS3):
            p = resize.resize_images_plan(srcs, dsts, algo)
            assert (p["launches_first"], p["launches_second"]) == (want, 1 if algo == LANCZOS3 else 0)
    # 300 images take the launches of 1
    srcs, dsts = [(9, 9, i % 4, 0) for i in range(300)], [(4, 4, i % 4, 0) for i in range(300)]
    p = resize.resize_images_plan(srcs, dsts, LANCZOS3)
    assert (p["launches_first"], p["launches_second"], p["sub_first"]) == (4, 1, [0, 300])


def test_plan_sub_batches_at_a_lowered_limit():
    srcs, dsts = ragged(2)  # colour types 2 3 0 1 2 3 0 1
    rows = [stride(d[0], s[2] + 1) * s[1] for s, d in zip(srcs, dsts)]
    assert rows == [64 * 23, 256 * 41, 16, 16 * 300, 784 * 5, 272 * 41, 304 * 7, 128 * 2]
    try:
        for limit in (1, 1472, 11968, 11984, 11983, 13536, 13535, 16784, 20720, 31872, 34000, 34256, 34255):
            jpeg.debug_configure("resize_batch_bytes=%d" % limit)
            p = resize.resize_images_plan(srcs, dsts, LANCZOS3)
            assert p == expected_plan(srcs, dsts, LANCZOS3, limit), limit
            for a, b in zip(p["sub_first"], p["sub_first"][1:]):
                assert b > a and p["mid_at"][a] == 0
                assert sum(rows[a:b]) <= limit or b == a + 1  # an image larger than the limit has a sub-batch to itself
            # every sub-batch launches for the pixel sizes IT holds, and once for its vertical pass
            subs = list(zip(p["sub_first"], p["sub_first"][1:]))
            assert p["launches_first"] == sum(len({srcs[i][2] for i in range(a, b)}) for a, b in subs) and p["launches_second"] == len(subs)
        jpeg.debug_configure("resize_batch_bytes=1")
        assert resize.resize_images_plan(srcs, dsts, LANCZOS3)["sub_first"] == list(range(9))
        jpeg.debug_configure("resize_batch_bytes=13536")  # images 0-2 hold 11984 bytes, 3-4 8720 (image 5 has 11152), 5-7 13536
        assert resize.resize_images_plan(srcs, dsts, LANCZOS3)["sub_first"] == [0, 3, 5, 8]
        jpeg.debug_configure("resize_batch_bytes=13535")
        assert resize.resize_images_plan(srcs, dsts, LANCZOS3)["sub_first"] == [0, 3, 5, 7, 8]
        # nearest and bilinear have no intermediate: never cut by it
        for algo in (NEAREST, BILINEAR):
            assert resize.resize_images_plan(srcs, dsts, algo)["sub_first"] == [0, 8]
    finally:
        jpeg.debug_configure(None)
    assert resize.resize_images_plan(srcs, dsts, LANCZOS3)["sub_first"] == [0, 8]  # the switch is back at its default


def test_plan_default_limit_is_256_mib():
    """4096 rows of 2^16 bytes are exactly 256 MiB: they fit; one more row does not"""
    dsts = [(1 << 16, 1, GRAY, 0)] * 2
    assert resize.resize_images_plan([(2, 4095, GRAY, 0), (2, 1, GRAY, 0)], dsts, LANCZOS3)["sub_first"] == [0, 2]
    assert resize.resize_images_plan([(2, 4095, GRAY, 0), (2, 2, GRAY, 0)], dsts, LANCZOS3)["sub_first"] == [0, 1, 2]


def test_plan_rows_of_tiles_are_capped():
    srcs, dsts = [(3, 262147, GRAY_ALPHA, 0), (5, 9, RGB, 0)], [(3, 262150, GRAY_ALPHA, 0), (300, 70000, RGB, 0)]
    for algo in (NEAREST, LANCZOS3):
        assert resize.resize_images_plan(srcs, dsts, algo) == expected_plan(srcs, dsts, algo)
    p = resize.resize_images_plan(srcs, dsts, LANCZOS3)
    assert p["tiles_first"] == [65535, 5 * 3] and p["tiles_second"] == [65535, 65535]
    assert resize.resize_images_plan(srcs, dsts, NEAREST)["tiles_first"] == [65535, 2 * 17500]
    small_s, small_d = ragged(1)
    try:
        for cap in (1, 2, 3, 70000):
            jpeg.debug_configure("resize_images_rows=%d" % cap)
            for algo in (BILINEAR, LANCZOS3):
                assert resize.resize_images_plan(small_s, small_d, algo) == expected_plan(small_s, small_d, algo, cap=min(cap, 65535)), (cap, algo)
        jpeg.debug_configure("resize_images_rows=1")
        p = resize.resize_images_plan(small_s, small_d, LANCZOS3)
        assert p["tiles_first"] == [ceil_div(w, 64) for w, _ in DST_SIZES]
    finally:
        jpeg.debug_configure(None)


def test_plan_a_launch_beyond_2_31_tiles_ends_the_sub_batch():
    """2^24 columns x 262140 rows are 65536 x 65535 point tiles — more than one launch holds — so the image's rows of tiles
    are cut to floor((2^31 - 1) / 65536) = 32767, which leaves room for 65535 tiles more in its launch"""
    huge = (2, 2, RGB, 0), (MAXD, 262140, RGB, 0)
    small = (2, 2, RGB, 0), (2, 2, RGB, 0)
    other = (2, 2, GRAY, 0), (2, 2, GRAY, 0)
    p = resize.resize_images_plan([huge[0], small[0]], [huge[1], small[1]], NEAREST)
    assert p["tiles_first"] == [65536 * 32767, 1] and p["sub_first"] == [0, 2] and p["launches_first"] == 1
    p = resize.resize_images_plan([huge[0], huge[0]], [huge[1], huge[1]], NEAREST)  # two such images cannot share a launch
    assert p["sub_first"] == [0, 1, 2] and p["launches_first"] == 2
    p = resize.resize_images_plan([huge[0], other[0]], [huge[1], other[1]], NEAREST)
    assert p["sub_first"] == [0, 2] and p["launches_first"] == 2
    # 2^31 - 1 tiles exactly fit one launch: 65536 x 32767 of one image and 1 x 65535 of another; one tile more does not
    tall = (2, 2, RGB, 0), (2, 262140, RGB, 0)
    p = resize.resize_images_plan([huge[0], tall[0]], [huge[1], tall[1]], NEAREST)
    assert p["sub_first"] == [0, 2] and sum(p["tiles_first"]) == (1 << 31) - 1 and p["launches_first"] == 1
    p = resize.resize_images_plan([huge[0], tall[0], small[0]], [huge[1], tall[1], small[1]], NEAREST)
    assert p["sub_first"] == [0, 2, 3] and p["launches_first"] == 2


# ---- the fitted sizes ----------------------------------------------------------------------------------------------------------
def js_round(x):
    """Math.round for x >= 0: a tie goes up"""
    f = math.floor(x)
    return f + 1 if x - f >= 0.5 else f


def fit_restated(sw, sh, box_w, box_h):
    """calculateResizeDimensions(srcWidth, srcHeight, maxWidth, maxHeight) of the reference's front end, in Python's f64"""
    aspect = sw / sh
    w, h = box_w, js_round(box_w / aspect)
    if h > box_h:
        h = box_h
        w = js_round(box_h * aspect)
    return max(1, w), max(1, h)


def fitted(sizes, box_w, box_h, no_enlarge=False, cts=None):
    images = [(w, h, ColorType(cts[i] if cts else RGB), 16 * i) for i, (w, h) in enumerate(sizes)]
    return resize.fit_images(images, box_w, box_h, no_enlarge)


def test_fit_worked_examples():
    assert fit_restated(3, 2, 2, 2) == (2, 1) and fit_restated(2, 3, 2, 2) == (1, 2)
    assert fit_restated(2, 1, 1, 1) == (1, 1) and fit_restated(2, 1, 3, 3) == (3, 2)  # 0.5 -> 1, 1.5 -> 2: a tie goes up
    assert fit_restated(1, 2, 5, 5) == (3, 5) and fit_restated(2, 5, 3, 3) == (1, 3)  # 2.5 -> 3; 1.2 -> 1
    assert fit_restated(1, 1000, 10, 10) == (1, 10) and fit_restated(1000, 1, 10, 10) == (10, 1)  # 0.01 -> 0 -> at least 1
    sizes = [(3, 2), (2, 3), (2, 1), (1, 2), (2, 5), (1, 1000), (1000, 1), (1920, 1080), (1080, 1920), (7, 7)]
    for box in ((2, 2), (1, 1), (3, 3), (5, 5), (10, 10), (320, 320), (320, 200), (200, 320), (1, 9), (9, 1)):
        got, _ = fitted(sizes, *box)
        assert [(w, h) for w, h, _, _ in got] == [fit_restated(w, h, *box) for w, h in sizes], box
        assert all(w <= box[0] and h <= box[1] for w, h, _, _ in got)


def test_fit_random_sizes_and_the_extremes():
    rng = random.Random(4711)
    pick = lambda: rng.choice([1, 2, 3, rng.randint(1, 40), rng.randint(1, 5000), rng.randint(1, MAXD), MAXD, MAXD - 1])  # noqa: E731
    for _ in range(40):
        sizes = [(pick(), pick()) for _ in range(50)] + [(1, pick()), (pick(), 1), (1, MAXD), (MAXD, 1), (MAXD, MAXD)]
        box = (pick(), pick())
        got, _ = fitted(sizes, *box)
        assert [(w, h) for w, h, _, _ in got] == [fit_restated(w, h, *box) for w, h in sizes], box
    for box in ((1, 1), (MAXD, MAXD), (1, MAXD), (MAXD, 1)):
        sizes = [(1, 1), (1, 7), (7, 1), (3, 2), (MAXD, 1), (1, MAXD), (MAXD, MAXD), (MAXD - 1, MAXD)]
        got, _ = fitted(sizes, *box, cts=[GRAY] * len(sizes))
        assert [(w, h) for w, h, _, _ in got] == [fit_restated(w, h, *box) for w, h in sizes], box
    assert fitted([(3, 2)], MAXD, MAXD, cts=[GRAY])[0][0][:2] == (MAXD, 11184811)  # 2^24 / 1.5 = 11184810.67


def test_fit_no_enlarge_layout_and_colour_types():
    sizes = [(10, 10), (30, 10), (10, 30), (20, 20), (21, 20), (5, 1), (3, 3)]
    cts = [RGB, RGBA, GRAY, GRAY_ALPHA, RGB, RGB, RGB]
    plain, total = fitted(sizes, 20, 20, cts=cts)
    kept, kept_total = fitted(sizes, 20, 20, no_enlarge=True, cts=cts)
    assert [(w, h) for w, h, _, _ in plain] == [(20, 20), (20, 7), (7, 20), (20, 20), (20, 19), (20, 4), (20, 20)]
    assert [(w, h) for w, h, _, _ in kept] == [(10, 10), (20, 7), (7, 20), (20, 20), (20, 19), (5, 1), (3, 3)]
    for got, end in ((plain, total), (kept, kept_total)):
        assert [ct for _, _, ct, _ in got] == [ColorType(c) for c in cts]  # every image keeps its own
        at = 0
        for w, h, ct, offset in got:  # the decode batch's layout: 16-byte starts, the total not rounded
            assert offset == at and offset % 16 == 0
            at = offset + w * h * (int(ct) + 1)
            last = at
            at = (at + 15) // 16 * 16
        assert end == last
    assert kept[-1][3] + 27 == kept_total and kept_total % 16 != 0
    # the records of a decode batch go in as they are, and what comes out is what encode_images and resize_images take
    arr = images_c([(30, 10, RGBA, 0), (10, 30, GRAY, 1200)])
    got, _ = resize.fit_images(arr, 20, 20)
    assert got == [(20, 7, ColorType.Rgba, 0), (7, 20, ColorType.Gray, 560)]
    assert resize.resize_images_plan(arr, got, BILINEAR)["sub_first"] == [0, 2]
    # in place, and `reserved` comes back as zeros
    L = _lib.load()
    arr[1].reserved[3] = 0xEE
    n = C.c_size_t()
    assert L.pixo_hip_resize_images_fit(arr, 2, 20, 20, 0, arr, C.byref(n)) == 0
    assert [(a.width, a.height, a.color_type, a.offset, bytes(a.reserved)) for a in arr] == [(20, 7, RGBA, 0, bytes(7)), (7, 20, GRAY, 560, bytes(7))]
    assert n.value == 700


def test_fit_refusals():
    L = _lib.load()
    good = images_c([(3, 3, RGB, 0), (5, 5, RGB, 0)])
    out, n = images_c([(77, 77, 0, 7)] * 2), C.c_size_t(99)

    def refused(status, cls, message, src=good, batch=2, box=(4, 4), dst=out, total=n):
        rc = L.pixo_hip_resize_images_fit(src, batch, box[0], box[1], 0, dst, C.byref(total) if total is not None else None)
        got = L.pixo_hip_last_error().decode()
        assert (rc, got) == (status, message), (rc, got)
        assert type(error.from_status(rc, got)) is cls
        assert [(o.width, o.offset) for o in out] == [(77, 7)] * 2 and n.value == 99  # nothing is written with a refusal

    null = "Compression error: null argument '%s'"
    refused(-6, error.CompressionError, null % "src_images", src=None, dst=None, total=None, batch=0, box=(0, 0))
    refused(-6, error.CompressionError, null % "dst_images", dst=None, total=None, batch=0, box=(0, 0))
    refused(-6, error.CompressionError, null % "total", total=None, batch=0, box=(0, 0))
    refused(-6, error.CompressionError, "Compression error: batch must be 1..65535", batch=0, box=(0, 0))
    refused(-6, error.CompressionError, "Compression error: batch must be 1..65535", batch=65536, box=(0, 0))
    bad = images_c([(3, 3, RGB, 0), (0, 5, RGB, 0)])
    refused(-1, error.InvalidDimensions, "Invalid image dimensions: 0x4", box=(0, 4), src=bad)
    refused(-1, error.InvalidDimensions, "Invalid image dimensions: 4x0", box=(4, 0), src=bad)
    refused(-4, error.ImageTooLarge, "Image %dx4 exceeds maximum dimension %d" % (MAXD + 1, MAXD), box=(MAXD + 1, 4), src=bad)
    refused(-4, error.ImageTooLarge, "Image 4x%d exceeds maximum dimension %d" % (MAXD + 1, MAXD), box=(4, MAXD + 1), src=bad)
    refused(-1, error.InvalidDimensions, "Invalid image dimensions: 0x5 (image 1)", src=bad)
    refused(-1, error.InvalidDimensions, "Invalid image dimensions: 5x0 (image 0)", src=images_c([(5, 0, RGB, 0), (0, 5, RGB, 0)]))
    refused(-4, error.ImageTooLarge, "Image %dx2 exceeds maximum dimension %d (image 1)" % (MAXD + 1, MAXD), src=images_c([(3, 3, RGB, 0), (MAXD + 1, 2, 9, 0)]))
    refused(-4, error.ImageTooLarge, "Image 2x%d exceeds maximum dimension %d (image 0)" % (MAXD + 1, MAXD), src=images_c([(2, MAXD + 1, RGB, 0), (0, 0, 0, 0)]))
    refused(-8, error.InvalidColorArgument, COLOR_MESSAGE % 4 + " (image 1)", src=images_c([(3, 3, RGB, 0), (3, 3, 4, 0)]))
    # offsets of the sources are not read: the layout is made anew
    got, total = resize.fit_images([(3, 3, ColorType.Rgb, 1 << 63), (5, 5, ColorType.Rgb, 5)], 4, 4)
    assert [g[3] for g in got] == [0, 48] and total == 96
    with pytest.raises(error.InvalidDimensions, match=r"^Invalid image dimensions: 0x4$"):
        resize.fit_images([(3, 3, RGB, 0)], 0, 4)
