"""The PNG decode batch entries (pixo_hip_png_decode_batch*, pixo_amd/csrc/png_decode_api.cpp) without a GPU: the ABI, every
phase-1 refusal with its status, class and exact message in the documented order, the layout the info entry reports against
values worked out here, and the plan entry — runs per image against a restatement of find_runs, launch counts, inflate
threads, sub-batch cuts, and the phase-2 refusals (what only the inflated streams show), which it raises as the decode
entries do."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

import png_decode_cases as PC
import png_decode_model as M
from pixo_amd import ColorType, _lib, decode, error, jpeg

NAMES = ("pixo_hip_png_decode_batch_info", "pixo_hip_png_decode_batch_device", "pixo_hip_png_decode_batch",
         "pixo_hip_debug_png_decode_batch_plan")
ENTRIES = ("info", "device", "host", "plan")
CLASS = {M.INVALID_DIMENSIONS: error.InvalidDimensions, M.IMAGE_TOO_LARGE: error.ImageTooLarge, M.INVALID_DECODE: error.InvalidDecode,
         M.UNSUPPORTED_DECODE: error.UnsupportedDecode}
HELD = np.zeros(64, np.uint8)  # something non-null to point at: no refusal below writes it
PASS_ROWS = 64
GOOD = [PC.make(5, 3, PC.RGB, 8, seed=1), PC.make(7, 2, PC.GRAY, 8, seed=2), PC.make(3, 3, PC.RGBA, 8, seed=3)]


def test_symbols_structs_and_constants():
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pixo_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"typedef struct pixo_png_file \{[^}]*\} pixo_png_file;", hdr)
    assert re.search(r"typedef struct pixo_png_image \{[^}]*\} pixo_png_image;", hdr)
    assert C.sizeof(_lib.PngFileC) == 16 and C.sizeof(_lib.PngImageC) == 24
    I = _lib.PngImageC
    assert (I.offset.offset, I.width.offset, I.height.offset, I.color_type.offset) == (0, 8, 12, 16)
    assert decode.ROUTES == {"PNG_DECODE_BATCH": 42} and decode.ROUTE_PNG_DECODE_BATCH == 1 << 42
    assert "PNG_DECODE_BATCH" not in jpeg.ROUTES
    assert re.search(r"#define PIXO_DECODE_ONE_THREAD 1u", hdr) and decode.ONE_THREAD == 1


def _files(pngs):
    """The C array and what keeps the bytes alive; an entry of None has a null `data`"""
    held = [None if p is None else np.frombuffer(p, np.uint8) for p in pngs]
    arr = (_lib.PngFileC * max(len(pngs), 1))()
    for i, f in enumerate(held):
        arr[i] = _lib.PngFileC(None, 5) if f is None else _lib.PngFileC(f.ctypes.data, f.size)
    return arr, held


def _images(n, fill=0xA5):
    images = (_lib.PngImageC * max(n, 1))()
    C.memset(images, fill, C.sizeof(images))
    return images


def _call(entry, pngs, batch=None, files="own", null=None, images=None, capacity=1 << 40, flags=0, d_pixels="held"):
    """One of the four entries.  null: the name of one trailing out-pointer to pass as null."""
    L = _lib.load()
    arr, held = _files(pngs)
    if files != "own":
        arr = files
    n = len(pngs) if batch is None else batch
    images = _images(n) if images is None else images

    def ptr(name, value):
        return None if null == name else value

    if entry == "info":
        total = C.c_size_t()
        return L.pixo_hip_png_decode_batch_info(arr, n, ptr("images", images), ptr("total", C.byref(total)))
    if entry == "device":
        d = HELD.ctypes.data if d_pixels == "held" else d_pixels
        return L.pixo_hip_png_decode_batch_device(arr, n, flags, d, capacity, ptr("images", images), None)
    if entry == "host":
        out, out_len = C.POINTER(C.c_uint8)(), C.c_size_t()
        return L.pixo_hip_png_decode_batch(arr, n, flags, ptr("out", C.byref(out)), ptr("out_len", C.byref(out_len)), ptr("images", images))
    sub_first, runs = (C.c_uint32 * (n + 1))(), (C.c_uint64 * max(n, 1))()
    subs, unfilter, convert, threads = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    return L.pixo_hip_debug_png_decode_batch_plan(arr, n, flags, ptr("sub_first", sub_first), ptr("sub_count", C.byref(subs)),
                                                  ptr("runs_per_image", runs), ptr("unfilter_launches", C.byref(unfilter)),
                                                  ptr("convert_launches", C.byref(convert)), ptr("threads", C.byref(threads)))


OUT_POINTERS = {"info": ("images", "total"), "device": ("images",), "host": ("out", "out_len", "images"),
                "plan": ("sub_first", "sub_count", "runs_per_image", "unfilter_launches", "convert_launches", "threads")}


def _refused(entry, status, cls, message, *args, **kw):
    rc = _call(entry, *args, **kw)
    got = _lib.load().pixo_hip_last_error().decode()
    assert (rc, got) == (status, message), (entry, rc, got)
    assert type(error.from_status(rc, got)) is cls


NULL = "Compression error: null argument '%s'"
RANGE = "Compression error: batch must be 1..65535"
BROKEN = list(PC.broken_cases())


@pytest.mark.parametrize("entry", ENTRIES)
def test_files_batch_and_out_pointers_in_that_order(entry):
    bad = BROKEN[0][1]
    big = (_lib.PngFileC * 65536)()  # (zeroed: were the batch accepted, image 0's null data would be refused instead)
    # files before batch, batch before the out-pointers, the out-pointers before any file
    _refused(entry, -6, error.CompressionError, NULL % "files", [bad], batch=0, files=None, null=OUT_POINTERS[entry][0])
    _refused(entry, -6, error.CompressionError, RANGE, [bad], batch=0, null=OUT_POINTERS[entry][0])
    _refused(entry, -6, error.CompressionError, RANGE, [], batch=65536, files=big)
    _refused(entry, -6, error.CompressionError, NULL % "data" + " (image 0)", [], batch=65535, files=big)
    for name in OUT_POINTERS[entry]:
        _refused(entry, -6, error.CompressionError, NULL % name, [bad, None], null=name)
    # a null data at index 2, behind good files; in front of a broken file 3
    _refused(entry, -6, error.CompressionError, NULL % "data" + " (image 2)", GOOD[:2] + [None, bad])


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name,png", BROKEN, ids=[n for n, _ in BROKEN])
def test_a_broken_file_is_refused_with_the_single_entrys_message(entry, name, png):
    want = PC.model(png)
    assert isinstance(want, M.DecodeError)
    with pytest.raises(error.Error) as single:
        decode.decode_png_info(png)
    assert str(single.value) == str(want)
    images = _images(3)
    before = bytes(images)
    _refused(entry, want.status, CLASS[want.status], str(want) + " (image 1)", [GOOD[0], png, GOOD[1]], images=images)
    assert bytes(images) == before  # untouched on a walk failure


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_lower_index_wins(entry):
    a, b = dict(BROKEN)["zero_width"], dict(BROKEN)["interlace_1"]
    _refused(entry, PC.model(b).status, error.UnsupportedDecode, str(PC.model(b)) + " (image 1)", [GOOD[0], b, GOOD[1], a])
    _refused(entry, PC.model(a).status, error.InvalidDimensions, str(PC.model(a)) + " (image 0)", [a, b])


def _claims(w, h, depth, ct):
    """A tiny file whose IHDR claims w x h: the walk accepts it (nothing is inflated in phase 1)"""
    return M.SIGNATURE + PC.chunk(b"IHDR", PC.ihdr(w, h, depth, ct)) + PC.chunk(b"IDAT", zlib.compress(b"\0" * 8)) + PC.chunk(b"IEND", b"")


def test_a_block_beyond_2_62_bytes_is_refused():
    huge = np.frombuffer(_claims(1 << 24, 1 << 24, 16, PC.RGBA), np.uint8)  # 2^48 pixels of 4 bytes: 2^50 bytes an image
    arr = (_lib.PngFileC * 4097)(*[_lib.PngFileC(huge.ctypes.data, huge.size)] * 4097)
    for entry in ENTRIES:
        images = _images(4097)
        before = bytes(images)
        _refused(entry, -6, error.CompressionError, "Compression error: batch output too large", [], batch=4097, files=arr, images=images)
        assert bytes(images) == before
    # 4096 of them are exactly 2^62 bytes: the layout is reported
    L, images, total = _lib.load(), _images(4096), C.c_size_t()
    assert L.pixo_hip_png_decode_batch_info(arr, 4096, images, C.byref(total)) == 0
    assert total.value == 1 << 62 and images[4095].offset == 4095 << 50 and images[4095].width == 1 << 24


def test_capacity_then_d_pixels():
    """The device entry's own two checks, behind the walks: the total in the single entry's words, `images` filled"""
    sizes = [5 * 3 * 3, 7 * 2, 3 * 3 * 4]
    total = 48 + 16 + 36
    images = _images(3)
    _refused("device", -9, error.BufferTooSmall, "output buffer too small: need %d bytes" % total, GOOD, capacity=total - 1, images=images)
    assert [(im.offset, im.width, im.height, im.color_type) for im in images] == [(0, 5, 3, 2), (48, 7, 2, 0), (64, 3, 3, 3)]
    _refused("device", -9, error.BufferTooSmall, "output buffer too small: need %d bytes" % total, GOOD, capacity=0, d_pixels=None)
    _refused("device", -6, error.CompressionError, NULL % "d_pixels", GOOD, capacity=total, d_pixels=None)
    assert sizes[0] == 45


# ---- info --------------------------------------------------------------------------------------------------------------------
MIXED = [
    (PC.make(1, 1, PC.GRAY, 8, seed=4), 1, 1, 1),                                    # 1 byte
    (PC.make(5, 3, PC.RGB, 8, seed=5), 5, 3, 3),                                     # 45 bytes
    (PC.make(64, 4, PC.RGBA, 8, seed=6), 64, 4, 4),                                  # a multiple of 16
    (PC.make(9, 5, PC.INDEXED, 4, seed=7, trns=bytes([0, 128])), 9, 5, 4),           # a palette with alpha: RGBA
    (PC.make(9, 5, PC.INDEXED, 2, seed=8, trns=bytes([255, 255])), 9, 5, 3),         # ... with an all-255 tRNS: RGB
    (PC.make(7, 3, PC.GRAY_ALPHA, 16, seed=9), 7, 3, 2),
    (PC.make(17, 2, PC.GRAY, 1, seed=10), 17, 2, 1),
]


def test_info_offsets_and_total():
    pngs = [m[0] for m in MIXED]
    at, want = 0, []
    for png, w, h, bpp in MIXED:
        mw, mh, px, ct = PC.model(png)
        assert (mw, mh, len(px), ct + 1) == (w, h, w * h * bpp, bpp)
        want.append((w, h, ColorType(ct), at))
        end = at + w * h * bpp
        at = (end + 15) // 16 * 16
    got, total = decode.decode_png_batch_info(pngs)
    assert got == want and total == end
    assert [o for _, _, _, o in want][:4] == [0, 16, 64, 64 + 1024]
    images, n = _images(len(pngs)), C.c_size_t()
    arr, held = _files(pngs)
    assert _lib.load().pixo_hip_png_decode_batch_info(arr, len(pngs), images, C.byref(n)) == 0
    assert all(bytes(im.reserved) == bytes(7) for im in images)
    # the info entry does not inflate: what only the stream shows passes it
    assert decode.decode_png_batch_info([PC.make(4, 4, PC.RGB, 8, filters=7, seed=1)])[1] == 48


def test_python_raises_the_errors_class():
    with pytest.raises(error.InvalidDimensions, match=r"^Invalid image dimensions: 0x1 \(image 1\)$"):
        decode.decode_png_batch_info([GOOD[0], dict(BROKEN)["zero_width"]])
    with pytest.raises(error.CompressionError, match="batch must be 1..65535"):
        decode.decode_png_batch([])
    with pytest.raises(error.InvalidDecode, match=r"^Decode error: not a PNG file \(image 0\)$"):
        decode.decode_png_batch([b"nothing"])
    with pytest.raises(error.UnsupportedDecode, match=r"\(image 2\)$"):
        decode.decode_png_batch_plan(GOOD[:2] + [dict(BROKEN)["interlace_1"]])


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def find_runs(filters):
    """png_decode_api.cpp find_runs: a row that does not read the row above (None, Sub) ends the run before it once that run
    has PASS_ROWS rows; the rest is the last run"""
    runs, run_at = [], 0
    for y, ft in enumerate(filters):
        if y > 0 and ft <= 1 and y - run_at >= PASS_ROWS:
            runs.append((run_at, y - run_at))
            run_at = y
    return runs + [(run_at, len(filters) - run_at)]


def _layouts():
    h = 131
    sub64 = [4] * h
    sub64[64], sub64[65] = 1, 0
    return [[4] * h, [0] * h, sub64, [y % 5 for y in range(h)]]


def test_plan_runs_per_image():
    layouts = _layouts()
    assert [len(find_runs(f)) for f in layouts[:2]] == [1, 3]  # all-Paeth: one run; all-None: rows 0-63, 64-127 and the remainder
    assert find_runs(layouts[2]) == [(0, 64), (64, 67)]
    pngs = [PC.make(67, 131, PC.RGB, 8, filters=f, seed=40 + i) for i, f in enumerate(layouts)]
    p = decode.decode_png_batch_plan(pngs)
    assert p["runs"] == [len(find_runs(f)) for f in layouts]
    assert p["sub_first"] == [0, 4] and (p["unfilter_launches"], p["convert_launches"]) == (1, 1)
    assert decode.pass_rows() == PASS_ROWS


def convert_kernel(ct, depth, w):
    """png_unfilter.hpp convert_kernel_of for a 16-byte aligned image: 0 sixteen bytes a thread, 1 byte-wise, 2 sample-wise"""
    if ct == PC.INDEXED or depth < 8:
        return 2
    return 0 if depth == 8 and (w * M.row_bytes(ct, 8, 1)) % 16 == 0 else 1


def test_plan_launch_counts():
    six = [(PC.GRAY, 8), (PC.GRAY, 16), (PC.RGB, 8), (PC.RGBA, 8), (PC.RGB, 16), (PC.RGBA, 16)]
    assert sorted(M.filter_unit(ct, d) for ct, d in six) == [1, 2, 3, 4, 6, 8]
    one = [PC.make(5, 4, PC.RGB, 8, seed=i) for i in range(5)]
    p = decode.decode_png_batch_plan(one)
    assert (p["unfilter_launches"], p["convert_launches"]) == (1, 1)
    all_six = [PC.make(5, 4, ct, d, seed=i) for i, (ct, d) in enumerate(six)]
    p = decode.decode_png_batch_plan(all_six)
    assert p["unfilter_launches"] == 6 and p["convert_launches"] == len({convert_kernel(ct, d, 5) for ct, d in six}) == 1
    # every convert kernel form, and units shared between colour types: palette and packed gray are unit 1
    mix = [(PC.RGBA, 8, 4), (PC.RGB, 8, 5), (PC.INDEXED, 4, 5), (PC.GRAY, 2, 5), (PC.GRAY, 8, 16), (PC.RGB, 16, 5)]
    p = decode.decode_png_batch_plan([PC.make(w, 4, ct, d, seed=i) for i, (ct, d, w) in enumerate(mix)])
    assert p["unfilter_launches"] == len({M.filter_unit(ct, d) for ct, d, _ in mix}) == 4
    assert p["convert_launches"] == len({convert_kernel(ct, d, w) for ct, d, w in mix}) == 3


def test_plan_threads():
    png = PC.make(3, 3, PC.GRAY, 8, seed=1)
    for n in (1, 2, 3, 7, 8, 9, 20):
        assert decode.decode_png_batch_plan([png] * n)["threads"] == min(n, 8)
        assert decode.decode_png_batch_plan([png] * n, one_thread=True)["threads"] == 1


def staging(w, h, ct, depth):
    """Device staging of an image: its stream (padded to 16) and its reconstructed rows at a pitch of a multiple of 16"""
    rb = M.row_bytes(ct, depth, w)
    return (h * (rb + 1) + 15) // 16 * 16 + h * ((rb + 15) // 16 * 16)


def expected_cuts(sizes, limit):
    """Greedy in order: an image joins the sub-batch while the staging stays within `limit`; every sub-batch holds one"""
    sub_first, held = [0], 0
    for i, s in enumerate(sizes):
        if i > sub_first[-1] and held + s > limit:
            sub_first.append(i)
            held = 0
        held += s
    return sub_first + [len(sizes)]


def test_plan_sub_batches_at_a_lowered_limit():
    shapes = [(5, 4, PC.RGB, 8), (33, 9, PC.RGBA, 8), (1, 1, PC.GRAY, 8), (67, 40, PC.RGB, 8), (9, 5, PC.INDEXED, 4), (5, 4, PC.RGB, 8)]
    sizes = [staging(*s) for s in shapes]
    assert sizes == [64 + 64, 1200 + 9 * 144, 16 + 16, 8080 + 40 * 208, 32 + 80, 128]
    pngs = [PC.make(w, h, ct, d, seed=50 + i) for i, (w, h, ct, d) in enumerate(shapes)]
    units = [M.filter_unit(ct, d) for _, _, ct, d in shapes]
    kernels = [convert_kernel(ct, d, w) for w, _, ct, d in shapes]
    try:
        for limit, cuts in ((1 << 30, [0, 6]), (sum(sizes), [0, 6]), (sum(sizes) - 1, [0, 5, 6]), (sizes[0] + sizes[1], [0, 2, 3, 4, 6]),
                            (sizes[0] + sizes[1] - 1, [0, 1, 3, 4, 6]), (1, [0, 1, 2, 3, 4, 5, 6])):
            jpeg.debug_configure("decode_batch_bytes=%d" % limit)
            p = decode.decode_png_batch_plan(pngs)
            assert p["sub_first"] == cuts == expected_cuts(sizes, limit), limit
            for a, b in zip(cuts, cuts[1:]):
                assert sum(sizes[a:b]) <= limit or b == a + 1  # an image above the limit is a sub-batch of its own
            # a launch per filter unit and per kernel form of every sub-batch
            assert p["unfilter_launches"] == sum(len(set(units[a:b])) for a, b in zip(cuts, cuts[1:]))
            assert p["convert_launches"] == sum(len(set(kernels[a:b])) for a, b in zip(cuts, cuts[1:]))
        assert sizes[3] > sizes[0] + sizes[1]  # ... image 3 at that limit: alone
    finally:
        jpeg.debug_configure(None)
    assert decode.decode_png_batch_plan(pngs)["sub_first"] == [0, 6]  # the switch is back at its default


# ---- phase 2 through the plan entry ----------------------------------------------------------------------------------------------
def bad_adler(png):
    """The file with the last byte of its one IDAT body (the stream's Adler-32) changed and the chunk's CRC made right again"""
    at = png.index(b"IDAT") - 4
    n = struct.unpack(">I", png[at:at + 4])[0]
    body = bytearray(png[at + 8:at + 8 + n])
    body[-1] ^= 0x5A
    return png[:at] + PC.chunk(b"IDAT", bytes(body)) + png[at + 12 + n:]


def test_phase_2_refusals_come_through_the_plan_entry():
    good = [PC.make(6, 5, PC.RGB, 8, seed=60 + i) for i in range(4)]
    filter7 = PC.make(6, 5, PC.RGB, 8, filters=[0, 2, 7, 4, 9], seed=64)
    no_plte = PC.make(6, 5, PC.INDEXED, 8, seed=65, no_plte=True)
    adler = bad_adler(good[3])
    for png, text in ((filter7, "invalid filter type: 7"), (no_plte, "missing PLTE chunk"), (adler, "Adler32 mismatch")):
        want = PC.model(png)
        assert isinstance(want, M.DecodeError) and text in str(want)
        decode.decode_png_batch_info([png])  # the walk accepts all three
    for one_thread in (False, True):
        with pytest.raises(error.InvalidDecode) as e:
            decode.decode_png_batch_plan([good[0], good[1], filter7, good[2]], one_thread=one_thread)
        assert str(e.value) == str(PC.model(filter7)) + " (image 2)"
        with pytest.raises(error.InvalidDecode) as e:
            decode.decode_png_batch_plan([good[0], no_plte, good[1], adler], one_thread=one_thread)
        assert str(e.value) == str(PC.model(no_plte)) + " (image 1)"
        with pytest.raises(error.InvalidDecode) as e:
            decode.decode_png_batch_plan([good[0], adler, good[1], no_plte], one_thread=one_thread)
        assert str(e.value) == str(PC.model(adler)) + " (image 1)"
    # many more files than threads, the faulty ones late and early: the lowest index decides every time
    many = [good[i % 4] for i in range(40)]
    many[37], many[11] = filter7, adler
    for _ in range(5):
        with pytest.raises(error.InvalidDecode) as e:
            decode.decode_png_batch_plan(many)
        assert str(e.value) == str(PC.model(adler)) + " (image 11)"
