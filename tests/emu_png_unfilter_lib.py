"""ctypes binding for tests/emu_png_unfilter/libpixo_emu_png_unfilter.so: the PNG decoder's per-byte arithmetic
(pixo_amd/csrc/png_unfilter_math.h) compiled for the host, built on demand.  Test harness only."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_png_unfilter")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_DIR, "libpixo_emu_png_unfilter.so"))
        L.emu_pngu_paeth.argtypes = [C.c_uint32] * 3
        L.emu_pngu_paeth.restype = C.c_uint32
        L.emu_pngu_reconstruct.argtypes = [C.c_uint32] * 5
        L.emu_pngu_reconstruct.restype = C.c_uint32
        L.emu_pngu_filter_unit.argtypes = [C.c_uint32] * 2
        L.emu_pngu_filter_unit.restype = C.c_uint32
        L.emu_pngu_row_bytes.argtypes = [C.c_uint32] * 3
        L.emu_pngu_row_bytes.restype = C.c_uint64
        L.emu_pngu_unfilter.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]
        L.emu_pngu_unfilter.restype = C.c_int64
        L.emu_pngu_convert.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        L.emu_pngu_convert.restype = C.c_uint32
        _LIB = L
    return _LIB


def unfilter(stream: bytes, height: int, rb: int, bpp: int):
    """-> (rows, first bad row or -1)"""
    s = np.frombuffer(stream, np.uint8)
    assert s.size == height * (rb + 1)
    rows = np.zeros(max(height * rb, 1), np.uint8)
    bad = lib().emu_pngu_unfilter(s.ctypes.data, height, rb, bpp, rows.ctypes.data)
    return rows[:height * rb].tobytes(), int(bad)


def convert(rows: bytes, width, height, color_type, depth, plte=None, trns=None) -> bytes:
    r = np.frombuffer(rows, np.uint8)
    p = np.frombuffer(plte or b"\0", np.uint8)
    t = np.frombuffer(trns or b"\0", np.uint8)
    out = np.zeros(width * height * 4, np.uint8)
    bpp = lib().emu_pngu_convert(r.ctypes.data, width, height, color_type, depth, p.ctypes.data, len(plte or b"") // 3, t.ctypes.data,
                                 len(trns or b""), out.ctypes.data)
    return out[:width * height * bpp].tobytes()
