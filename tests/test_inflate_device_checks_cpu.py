"""The device inflate's public surface without a GPU (PIXO_DECODE_DEVICE_INFLATE; pixo_amd/csrc/png_decode_api.cpp): the symbols,
the flag and the route bits in the header, the loader and the library; the refusals that must not need a device — every
argument check, every phase-1 refusal and the zlib header refusals, with the status, class and message the call has without the
flag and the lowest index deciding; and the plan entry, which ignores the flag."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

import inflate_cases as IC
import png_decode_cases as PC
import png_decode_model as M
from pixo_amd import _lib, decode, error, jpeg

NEW = ("pixo_hip_png_inflate_step_tokens", "pixo_hip_png_inflate_window_bytes", "pixo_hip_png_inflate_far_distance",
       "pixo_hip_png_inflate_stored_chunk", "pixo_hip_debug_zlib_inflate_batch_device")
HELD = np.zeros(64, np.uint8)
GOOD = [PC.make(5, 3, PC.RGB, 8, seed=1), PC.make(7, 2, PC.GRAY, 8, seed=2), PC.make(3, 3, PC.RGBA, 8, seed=3)]
BROKEN = list(PC.broken_cases())
CLASS = {M.INVALID_DIMENSIONS: error.InvalidDimensions, M.IMAGE_TOO_LARGE: error.ImageTooLarge, M.INVALID_DECODE: error.InvalidDecode,
         M.UNSUPPORTED_DECODE: error.UnsupportedDecode}


def header():
    return open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pixo_hip.h")).read()


def test_symbols_flag_and_routes():
    hdr, lib = header(), _lib.load()
    for name in NEW:
        assert re.search(r"\b(int|uint32_t) %s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define PIXO_DECODE_DEVICE_INFLATE 2u", hdr) and decode.DEVICE_INFLATE == 2
    assert re.search(r"#define PIXO_DECODE_ONE_THREAD 1u", hdr) and decode.ONE_THREAD == 1
    assert decode.INFLATE_ROUTES == {"PNG_INFLATE_DEVICE": 43, "PNG_INFLATE_HOST_REDO": 44}
    routes = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "routes.hpp")).read()
    for name, bit in decode.INFLATE_ROUTES.items():
        assert re.search(r"\b%s = 1ull << %d," % (name, bit), routes), name
    # the complete lists other tests pin stay as they are
    assert decode.ROUTES == {"PNG_DECODE_BATCH": 42}
    assert not set(decode.INFLATE_ROUTES) & set(jpeg.ROUTES) and max(jpeg.ROUTES.values()) < 42
    assert (decode.inflate_step_tokens(), decode.inflate_window_bytes()) == (64, 32768)
    assert decode.inflate_far_distance() == 32768 - 64 * 258 and decode.inflate_stored_chunk() == 4096


def _files(pngs):
    held = [np.frombuffer(p, np.uint8) for p in pngs]
    arr = (_lib.PngFileC * max(len(pngs), 1))()
    for i, f in enumerate(held):
        arr[i] = _lib.PngFileC(f.ctypes.data, f.size)
    return arr, held


def _call(entry, pngs, flags, capacity=1 << 40):
    """-> (status, message): the device entry with a HOST address for d_pixels (no refusal below touches it), or the host entry"""
    L = _lib.load()
    arr, held = _files(pngs)
    images = (_lib.PngImageC * max(len(pngs), 1))()
    if entry == "device":
        rc = L.pixo_hip_png_decode_batch_device(arr, len(pngs), flags, HELD.ctypes.data, capacity, images, None)
    else:
        out, out_len = C.POINTER(C.c_uint8)(), C.c_size_t()
        rc = L.pixo_hip_png_decode_batch(arr, len(pngs), flags, C.byref(out), C.byref(out_len), images)
    return rc, L.pixo_hip_last_error().decode()


FLAGS = (decode.DEVICE_INFLATE, decode.DEVICE_INFLATE | decode.ONE_THREAD)


@pytest.mark.parametrize("entry", ("device", "host"))
@pytest.mark.parametrize("name,png", BROKEN, ids=[n for n, _ in BROKEN])
def test_phase_1_refusals_are_todays(entry, name, png):
    want = PC.model(png)
    for flags in FLAGS:
        rc, msg = _call(entry, [GOOD[0], png, GOOD[1]], flags)
        assert (rc, msg) == (want.status, str(want) + " (image 1)")
        assert type(error.from_status(rc, msg)) is CLASS[want.status]


def test_argument_checks_are_todays():
    L = _lib.load()
    images = (_lib.PngImageC * 1)()
    for flags in FLAGS:
        assert L.pixo_hip_png_decode_batch_device(None, 1, flags, HELD.ctypes.data, 64, images, None) == -6
        assert L.pixo_hip_last_error().decode() == "Compression error: null argument 'files'"
        arr, held = _files(GOOD)
        assert L.pixo_hip_png_decode_batch_device(arr, 0, flags, HELD.ctypes.data, 64, images, None) == -6
        assert L.pixo_hip_last_error().decode() == "Compression error: batch must be 1..65535"
        assert _call("device", GOOD, flags, capacity=99) == (-9, "output buffer too small: need 100 bytes")


def with_idat(png, body):
    """The file with its one IDAT body replaced (the chunk's CRC made right)"""
    at = png.index(b"IDAT") - 4
    n = struct.unpack(">I", png[at:at + 4])[0]
    return png[:at] + PC.chunk(b"IDAT", body) + png[at + 12 + n:]


def zlib_header_cases():
    good = GOOD[0]
    z = zlib.compress(b"\0" * 48)
    yield "too_short", with_idat(good, b"\x78\x9c\x03\x00\x00"), M.INVALID_DECODE, "Decode error: zlib stream too short"
    yield "method", with_idat(good, b"\x77\x9c" + z[2:]), M.INVALID_DECODE, "Decode error: invalid zlib compression method"
    yield "checksum", with_idat(good, b"\x78\x9d" + z[2:]), M.INVALID_DECODE, "Decode error: invalid zlib header checksum"
    yield "dictionary", with_idat(good, b"\x78\xbb" + z[2:]), M.UNSUPPORTED_DECODE, "Unsupported: preset dictionary not supported"


ZLIB_HEADERS = list(zlib_header_cases())


@pytest.mark.parametrize("entry", ("device", "host"))
@pytest.mark.parametrize("name,png,status,message", ZLIB_HEADERS, ids=[c[0] for c in ZLIB_HEADERS])
def test_zlib_header_refusals_need_no_gpu_and_are_todays(entry, name, png, status, message):
    with pytest.raises(error.Error) as plain:
        decode.decode_png_batch_plan([GOOD[1], png, GOOD[2]])  # (the call without the flag refuses with the plan entry's words)
    assert str(plain.value) == message + " (image 1)"
    for flags in FLAGS:
        rc, msg = _call(entry, [GOOD[1], png, GOOD[2]], flags)
        assert (rc, msg) == (status, message + " (image 1)")
        assert type(error.from_status(rc, msg)) is CLASS[status]


@pytest.mark.parametrize("entry", ("device", "host"))
def test_a_file_in_front_of_a_bad_zlib_header_that_fails_later_checks_still_decides(entry):
    """Without the flag the failing file with the lowest index decides, whatever its fault: a bad Adler-32 or a filter byte above 4
    at index 0 is reported, not the bad zlib header at index 2 — and that needs no GPU either"""
    filter7 = PC.make(6, 5, PC.RGB, 8, filters=[0, 2, 7, 4, 9], seed=64)
    body = zlib.compress(b"\0" * 48)
    bad_adler = with_idat(GOOD[0], body[:-1] + bytes([body[-1] ^ 0x5A]))
    head = ZLIB_HEADERS[1][1]
    for first in (filter7, bad_adler):
        with pytest.raises(error.InvalidDecode) as plain:
            decode.decode_png_batch_plan([first, GOOD[1], head])
        assert str(plain.value).endswith(" (image 0)")
        for flags in FLAGS:
            assert _call(entry, [first, GOOD[1], head], flags) == (M.INVALID_DECODE, str(plain.value))


def test_the_plan_entry_ignores_the_flag():
    pngs = [PC.make(67, 131, PC.RGB, 8, filters=f, seed=40 + i) for i, f in enumerate(([4] * 131, [0] * 131, [y % 5 for y in range(131)]))]
    L = _lib.load()
    arr, held = _files(pngs)
    got = []
    for flags in (0, decode.DEVICE_INFLATE, decode.ONE_THREAD, decode.ONE_THREAD | decode.DEVICE_INFLATE):
        sub_first, runs = (C.c_uint32 * 4)(), (C.c_uint64 * 3)()
        subs, unfilter, convert, threads = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        assert L.pixo_hip_debug_png_decode_batch_plan(arr, 3, flags, sub_first, C.byref(subs), runs, C.byref(unfilter), C.byref(convert),
                                                      C.byref(threads)) == 0
        got.append((list(sub_first[:subs.value + 1]), list(runs), unfilter.value, convert.value, threads.value))
    assert got[0] == got[1] and got[2] == got[3] and got[0][:4] == got[2][:4] and (got[0][4], got[2][4]) == (3, 1)
    assert got[0][1] == [1, 3, 3]


def test_the_debug_entrys_argument_checks():
    L = _lib.load()
    z = np.frombuffer(zlib.compress(b"abc"), np.uint8)
    arr = (_lib.PngFileC * 1)(_lib.PngFileC(z.ctypes.data, z.size))
    one64, one32, ms = (C.c_uint64 * 1)(3), (C.c_uint32 * 1)(), C.c_double()
    args = [arr, 1, one64, HELD.ctypes.data, (C.c_uint64 * 1)(0), one32, (C.c_uint64 * 1)(), (C.c_uint32 * 1)(), C.byref(ms)]
    names = ["streams", None, "expected", None, "out_at", "verdict", "produced", "adler", "kernel_ms"]
    for i, name in enumerate(names):
        if name is None:
            continue
        a = list(args)
        a[i] = None
        assert L.pixo_hip_debug_zlib_inflate_batch_device(*a) == -6
        assert L.pixo_hip_last_error().decode() == "Compression error: null argument '%s'" % name
    a = list(args)
    a[1] = 0
    assert L.pixo_hip_debug_zlib_inflate_batch_device(*a) == -6 and "batch must be 1..65535" in L.pixo_hip_last_error().decode()


def test_the_cases_name_every_boundary_once():
    cases = IC.cases(decode.inflate_step_tokens(), decode.inflate_window_bytes(), decode.inflate_far_distance(), decode.inflate_stored_chunk())
    names = [c["name"] for c in cases]
    for part in ("tiny_empty", "stored_0_bytes", "stored_65535_bytes", "mid_byte", "stored_fixed_dynamic", "z_full_flush", "match_258_at_distance_1",
                 "distance_32768_at_offset_32768", "one_past", "16_byte", "literal_tokens_63", "literal_tokens_64", "literal_tokens_65",
                 "same_step", "window_output_32767", "window_output_32768", "window_output_32769", "window_output_65537", "15_bit",
                 "single_distance_code", "oversubscribed", "z_fixed", "z_huffman_only", "z_rle", "z_level_1", "z_level_9", "junk", "one_short",
                 "one_long", "error_reserved_block_type", "error_invalid_Huffman_code"):
        assert any(part in n for n in names), part
    assert sum(n.startswith("error_") for n in names) == len(IC.error_streams()) + 1
