"""The resize batch entries (pixo_hip_resize_batch*, pixo_amd/csrc/resize_api.cpp) without a GPU: the ABI, every refusal with
its status, class and exact message in the documented order (all before anything is enqueued), the Python size checks, and
the plan — sub-batches, offsets into the intermediate, LDS staging per image, shared axis tables — against values worked out
here from the launch arithmetic tests/resize_reach_cases.py restates."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resize_cases as RC
import resize_reach_cases as RR
from pixo_amd import _lib, error, jpeg, resize

NAMES = ("pixo_hip_resize_batch_device", "pixo_hip_resize_batch", "pixo_hip_debug_resize_batch_plan")
NEAREST, BILINEAR, LANCZOS3 = 0, 1, 2
RGB = 2
MAXD = 1 << 24
HELD = np.zeros(4, np.uint8)  # something non-null to point at: no refusal below reads it


def test_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pixo_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"typedef struct pixo_resize_source \{[^}]*\} pixo_resize_source;", hdr)
    assert resize.ROUTES["RESIZE_BATCH"] == 41 and resize.ROUTE_RESIZE_BATCH == 1 << 41
    assert "RESIZE_BATCH" not in jpeg.ROUTES


def test_source_struct_layout():
    assert C.sizeof(_lib.ResizeSourceC) == 16
    assert (_lib.ResizeSourceC.pixels.offset, _lib.ResizeSourceC.width.offset, _lib.ResizeSourceC.height.offset) == (0, 8, 12)


def _sources(sizes, pixels=None):
    arr = (_lib.ResizeSourceC * max(len(sizes), 1))()
    for i, (w, h) in enumerate(sizes):
        arr[i] = _lib.ResizeSourceC(HELD.ctypes.data if pixels is None else pixels[i], w, h)
    return arr


def _call(entry, sizes, dw, dh, ct, algo, pixels=None, batch=None, sources="own", last=True):
    """One of the three entries with good trailing pointers unless `last` is False (then the first of them is null)"""
    L = _lib.load()
    src = _sources(sizes, pixels) if sources == "own" else sources
    n = len(sizes) if batch is None else batch
    if entry == "device":
        return L.pixo_hip_resize_batch_device(src, n, dw, dh, ct, algo, HELD.ctypes.data if last else None, None)
    if entry == "host":
        out, out_len = C.POINTER(C.c_uint8)(), C.c_size_t()
        return L.pixo_hip_resize_batch(src, n, dw, dh, ct, algo, C.byref(out) if last else None, C.byref(out_len))
    sub_first, mid_at, use_lds = (C.c_uint32 * (n + 1))(), (C.c_uint64 * max(n, 1))(), (C.c_uint8 * max(n, 1))()
    subs, tables = C.c_uint32(), C.c_uint32()
    return L.pixo_hip_debug_resize_batch_plan(src, n, dw, dh, ct, algo, sub_first if last else None, C.byref(subs), mid_at, use_lds, C.byref(tables))


def _refused(entry, status, cls, message, *args, **kw):
    rc = _call(entry, *args, **kw)
    got = _lib.load().pixo_hip_last_error().decode()
    assert (rc, got) == (status, message), (entry, rc, got)
    assert type(error.from_status(rc, got)) is cls


ENTRIES = ("device", "host", "plan")
GOOD = [(37, 23), (64, 41)]

# (sizes, dw, dh, colour type, algorithm) -> status, class, the single entry's message, the image it is reported for
REFUSALS = [
    ((GOOD + [(0, 5)], 17, 13, RGB, LANCZOS3), -1, error.InvalidDimensions, "Invalid image dimensions: 0x5", 2),
    ((GOOD + [(5, 0)], 17, 13, RGB, NEAREST), -1, error.InvalidDimensions, "Invalid image dimensions: 5x0", 2),
    ((GOOD, 0, 13, RGB, BILINEAR), -1, error.InvalidDimensions, "Invalid image dimensions: 0x13", 0),
    ((GOOD, 17, 0, RGB, LANCZOS3), -1, error.InvalidDimensions, "Invalid image dimensions: 17x0", 0),
    (([(3, 3), (MAXD + 1, 2)], 17, 13, RGB, NEAREST), -4, error.ImageTooLarge, "Image %dx13 exceeds maximum dimension %d" % (MAXD + 1, MAXD), 1),
    (([(3, 3), (2, MAXD + 1)], 17, 13, RGB, NEAREST), -4, error.ImageTooLarge, "Image 17x%d exceeds maximum dimension %d" % (MAXD + 1, MAXD), 1),
    ((GOOD, MAXD + 1, 13, 0, BILINEAR), -4, error.ImageTooLarge, "Image %dx23 exceeds maximum dimension %d" % (MAXD + 1, MAXD), 0),
    ((GOOD, 17, 13, 4, LANCZOS3), -8, error.InvalidColorArgument, "Invalid color type: 4. Expected 0 (Gray), 1 (GrayAlpha), 2 (Rgb), or 3 (Rgba)", 0),
    ((GOOD, 17, 13, RGB, 3), -8, error.InvalidColorArgument, "Invalid resize algorithm: 3. Expected 0 (Nearest), 1 (Bilinear), or 2 (Lanczos3)", 0),
    # the single entry's order within one image: source size, destination size, too large, colour type, algorithm
    (([(0, 0)], 0, 0, 9, 9), -1, error.InvalidDimensions, "Invalid image dimensions: 0x0", 0),
    (([(1, 1)], MAXD + 1, 1, 9, 9), -4, error.ImageTooLarge, "Image %dx1 exceeds maximum dimension %d" % (MAXD + 1, MAXD), 0),
    (([(1, 1)], 1, 1, 9, 9), -8, error.InvalidColorArgument, "Invalid color type: 9. Expected 0 (Gray), 1 (GrayAlpha), 2 (Rgb), or 3 (Rgba)", 0),
]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("r", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_a_source_is_refused_with_the_single_entrys_status_and_message(entry, r):
    args, status, cls, message, image = r
    _refused(entry, status, cls, "%s (image %d)" % (message, image), *args)


def test_the_message_is_the_single_entrys():
    """... which is pinned to the reference by tests/golden/resize_cases.json: same call through pixo_hip_resize_device"""
    L = _lib.load()
    for args, status, _, message, image in REFUSALS:
        sizes, dw, dh, ct, algo = args
        o = _lib.ResizeOptionsC(sizes[image][0], sizes[image][1], dw, dh, ct, algo)
        assert L.pixo_hip_resize_device(HELD.ctypes.data, C.byref(o), HELD.ctypes.data, None) == status
        assert L.pixo_hip_last_error().decode() == message


@pytest.mark.parametrize("entry", ENTRIES)
def test_order_of_refusals(entry):
    bad = (0, 7)
    # a bad image at index 2 behind a good 0 and 1
    _refused(entry, -1, error.InvalidDimensions, "Invalid image dimensions: 0x7 (image 2)", GOOD + [bad, (5, 5)], 17, 13, RGB, LANCZOS3)
    # a bad image 0 wins over a bad image 3
    _refused(entry, -4, error.ImageTooLarge, "Image %dx13 exceeds maximum dimension %d (image 0)" % (MAXD + 1, MAXD),
             [(MAXD + 1, 1)] + GOOD + [bad], 17, 13, RGB, LANCZOS3)
    # sources before batch, batch before any image, images before pixels, pixels before the entry's own pointers
    _refused(entry, -6, error.CompressionError, "Compression error: null argument 'sources'", [bad], 17, 13, RGB, 0, batch=0, sources=None)
    _refused(entry, -6, error.CompressionError, "Compression error: batch must be 1..65535", [bad], 17, 13, RGB, 0, batch=0)
    _refused(entry, -1, error.InvalidDimensions, "Invalid image dimensions: 0x7 (image 1)", [(5, 5), bad], 17, 13, RGB, 0, pixels=[0, 0], last=False)
    if entry != "plan":  # (the plan entry ignores `pixels`)
        _refused(entry, -6, error.CompressionError, "Compression error: null argument 'pixels' (image 1)", GOOD + [(5, 5)], 17, 13, RGB, 0,
                 pixels=[HELD.ctypes.data, 0, 0], last=False)


@pytest.mark.parametrize("entry", ENTRIES)
def test_batch_out_of_range_and_null_pointers(entry):
    big = (_lib.ResizeSourceC * 65536)()  # (zeroed: were the batch accepted, image 0 would be refused instead)
    _refused(entry, -6, error.CompressionError, "Compression error: batch must be 1..65535", [], 17, 13, RGB, 0, batch=0)
    _refused(entry, -6, error.CompressionError, "Compression error: batch must be 1..65535", [], 17, 13, RGB, 0, batch=65536, sources=big)
    _refused(entry, -1, error.InvalidDimensions, "Invalid image dimensions: 0x0 (image 0)", [], 17, 13, RGB, 0, batch=65535, sources=big)
    _refused(entry, -6, error.CompressionError, "Compression error: null argument 'sources'", GOOD, 17, 13, RGB, 0, sources=None)
    last = {"device": "d_dst", "host": "out", "plan": "sub_first"}[entry]
    _refused(entry, -6, error.CompressionError, "Compression error: null argument '%s'" % last, GOOD, 17, 13, RGB, 0, last=False)
    if entry != "plan":
        _refused(entry, -6, error.CompressionError, "Compression error: null argument 'pixels' (image 0)", GOOD, 17, 13, RGB, 0,
                 pixels=[0, HELD.ctypes.data])
    if entry == "host":
        L, out = _lib.load(), C.POINTER(C.c_uint8)()
        assert L.pixo_hip_resize_batch(_sources(GOOD), 2, 17, 13, RGB, 0, C.byref(out), None) == -6
        assert L.pixo_hip_last_error().decode() == "Compression error: null argument 'out_len'"


def test_python_raises_the_errors_class():
    with pytest.raises(error.InvalidDimensions, match=r"^Invalid image dimensions: 0x5 \(image 1\)$"):
        resize.resize_batch_device([(HELD.ctypes.data, 3, 3), (HELD.ctypes.data, 0, 5)], 4, 4, RGB, LANCZOS3, HELD.ctypes.data)
    with pytest.raises(error.InvalidColorArgument, match=r"^Invalid color type: 7\. .* \(image 0\)$"):
        resize.resize_batch([(np.zeros(27, np.uint8), 3, 3)], 4, 4, 7, BILINEAR)
    with pytest.raises(error.CompressionError, match="batch must be 1..65535"):
        resize.resize_batch([], 4, 4, RGB, BILINEAR)
    with pytest.raises(error.ImageTooLarge, match=r"\(image 0\)$"):
        resize.resize_batch_plan([(MAXD + 1, 1)], 4, 4, RGB, NEAREST)


def test_python_size_checks_raise_value_error():
    torch = pytest.importorskip("torch")
    good, short = torch.zeros(3 * 3 * 3, dtype=torch.uint8), torch.zeros(3 * 3 * 3 - 1, dtype=torch.uint8)
    dst = torch.zeros(2 * 4 * 4 * 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="source 1 of 3x3 needs 27 bytes of pixels, it holds 26"):
        resize.resize_batch_device([(good, 3, 3), (short, 3, 3)], 4, 4, RGB, NEAREST, dst)
    with pytest.raises(ValueError, match="a batch of 2 images of 4x4 needs 96 bytes of output, the tensor holds 95"):
        resize.resize_batch_device([(good, 3, 3), (good, 3, 3)], 4, 4, RGB, NEAREST, dst[:95])
    with pytest.raises(ValueError, match="a batch of 1 images of 4x4 needs 48 bytes of output, the tensor holds 96"):
        resize.resize_batch_device([(good, 3, 3)], 4, 4, RGB, NEAREST, dst)
    with pytest.raises(ValueError, match="source 0 of 3x3 needs 27 bytes of pixels, it holds 28"):
        resize.resize_batch([(np.zeros(28, np.uint8), 3, 3)], 4, 4, RGB, NEAREST)


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def stride(dw, bpp):
    return (dw * bpp + 15) // 16 * 16


def expected_lds(sw, dw, bpp):
    return RR.max_span(*RR.taps(sw, dw)) * bpp + 8 <= RR.SEG_BYTES


def expected_plan(sizes, dw, dh, ct, limit=256 << 20):
    """Greedy in order: an image joins the sub-batch while the intermediates stay within `limit`; every sub-batch holds one"""
    bpp = RC.BPP[ct]
    sub_first, mid_at, held = [0], [], 0
    for i, (w, h) in enumerate(sizes):
        rows = stride(dw, bpp) * h
        if i > sub_first[-1] and held + rows > limit:
            sub_first.append(i)
            held = 0
        mid_at.append(held)
        held += rows
    return dict(sub_first=sub_first + [len(sizes)], mid_at=mid_at, use_lds=[expected_lds(w, dw, bpp) for w, _ in sizes],
                axis_tables=len({w for w, _ in sizes}) + len({h for _, h in sizes}))


RAGGED = [(37, 23), (64, 41), (1, 1), (5, 300), (300, 5), (64, 41), (129, 7)]


def test_plan_equal_sources_build_two_tables():
    p = resize.resize_batch_plan([(64, 41)] * 5, 17, 13, RGB, LANCZOS3)
    assert p["axis_tables"] == 2 and p["sub_first"] == [0, 5]
    assert p["mid_at"] == [i * 64 * 41 for i in range(5)]  # 17 * 3 = 51 bytes a row, padded to 64
    # a square source still has one table per axis
    assert resize.resize_batch_plan([(64, 64)] * 2, 64, 64, 0, LANCZOS3)["axis_tables"] == 2


def test_plan_a_repeated_size_is_shared():
    for ct in range(4):
        p = resize.resize_batch_plan(RAGGED, 17, 13, ct, LANCZOS3)
        assert p == expected_plan(RAGGED, 17, 13, ct)
        assert p["axis_tables"] == 6 + 6  # widths 37 64 1 5 300 129, heights 23 41 1 300 5 7
    # a width met as a height is another axis
    assert resize.resize_batch_plan([(5, 9), (9, 5)], 3, 3, 0, LANCZOS3)["axis_tables"] == 4
    assert resize.resize_batch_plan([(5, 9), (5, 11), (7, 9)], 3, 3, 0, LANCZOS3)["axis_tables"] == 4


def test_plan_point_algorithms_have_no_tables_and_are_never_cut():
    jpeg.debug_configure("resize_batch_bytes=16")
    try:
        for algo in (NEAREST, BILINEAR):
            p = resize.resize_batch_plan(RAGGED, 17, 13, RGB, algo)
            assert p == dict(sub_first=[0, len(RAGGED)], mid_at=[0] * len(RAGGED), use_lds=[False] * len(RAGGED), axis_tables=0)
    finally:
        jpeg.debug_configure(None)


def test_plan_use_lds_on_both_sides_of_the_threshold():
    """The widths of resize_reach_cases.A_CASES: with dst_w = 1 the one tile spans the whole row, sw * bpp + 8 bytes staged"""
    for ct in range(4):
        pairs = [c for c in RR.A_CASES if c["color_type"] == ct and c["dw"] == 1 and c["staged_bytes"] in (8192, 8192 + RC.BPP[ct])]
        assert {c["use_lds"] for c in pairs} == {False, True}
        sizes = [(c["sw"], c["sh"]) for c in pairs] + [(3, 3)]
        p = resize.resize_batch_plan(sizes, 1, 3, ct, LANCZOS3)
        assert p["use_lds"] == [c["use_lds"] for c in pairs] + [True]
        assert p["use_lds"] == [expected_lds(w, 1, RC.BPP[ct]) for w, _ in sizes]
        assert p == expected_plan(sizes, 1, 3, ct)
    # the pixel size alone moves one width across the threshold
    assert [resize.resize_batch_plan([(2047, 5)], 1, 3, ct, LANCZOS3)["use_lds"][0] for ct in range(4)] == [True, True, True, False]


def test_plan_mid_at_is_aligned_and_does_not_overlap():
    for dw, dh, ct in ((17, 13, 2), (64, 41, 1), (3, 3, 2), (1, 1, 0), (5, 2, 3)):
        p = resize.resize_batch_plan(RAGGED, dw, dh, ct, LANCZOS3)
        assert p["sub_first"] == [0, len(RAGGED)]
        assert all(at % 16 == 0 for at in p["mid_at"])
        ends = [at + stride(dw, RC.BPP[ct]) * h for at, (_, h) in zip(p["mid_at"], RAGGED)]
        assert p["mid_at"][0] == 0 and p["mid_at"][1:] == ends[:-1]


def test_plan_sub_batches_at_a_lowered_limit():
    dw, dh, ct = 17, 13, RGB  # 64 bytes a row of the intermediate
    rows = [64 * h for _, h in RAGGED]  # 1472 2624 64 19200 320 2624 448
    try:
        for limit, cuts in ((4096, [0, 2, 3, 4, 7]), (4160, [0, 3, 4, 7]), (19200, [0, 3, 4, 7]), (19199, [0, 3, 4, 7]),
                            (23360, [0, 4, 7]), (26752, [0, 7]), (26751, [0, 6, 7]), (1, [0, 1, 2, 3, 4, 5, 6, 7])):
            jpeg.debug_configure("resize_batch_bytes=%d" % limit)
            p = resize.resize_batch_plan(RAGGED, dw, dh, ct, LANCZOS3)
            assert p == expected_plan(RAGGED, dw, dh, ct, limit), limit
            assert p["sub_first"] == cuts, limit
            for a, b in zip(p["sub_first"], p["sub_first"][1:]):
                assert b > a and p["mid_at"][a] == 0
                assert sum(rows[a:b]) <= limit or b == a + 1  # an image larger than the limit has a sub-batch to itself
        # ... image 3 (19,200 bytes) at a limit of 4,160: alone, its neighbours not
        jpeg.debug_configure("resize_batch_bytes=4160")
        p = resize.resize_batch_plan(RAGGED, dw, dh, ct, LANCZOS3)
        assert [p["sub_first"][k] for k in (1, 2)] == [3, 4] and rows[3] > 4160
    finally:
        jpeg.debug_configure(None)
    assert resize.resize_batch_plan(RAGGED, dw, dh, ct, LANCZOS3)["sub_first"] == [0, 7]  # the switch is back at its default


def test_plan_default_limit_is_256_mib():
    """4096 rows of 2^16 bytes are exactly 256 MiB: they fit; one more row does not"""
    assert resize.resize_batch_plan([(2, 4095), (2, 1)], 1 << 16, 1, 0, LANCZOS3)["sub_first"] == [0, 2]
    assert resize.resize_batch_plan([(2, 4095), (2, 2)], 1 << 16, 1, 0, LANCZOS3)["sub_first"] == [0, 1, 2]
