"""ctypes binding for tests/emu_png_reduce/libpixo_emu_png_reduce.so: the arithmetic of the PNG reduction kernels
(pixo_amd/csrc/png_reduce_math.h) compiled for the host, built on demand.  Test harness only."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_png_reduce")
_LIB = None
FORM_INDEX, FORM_GRAY, FORM_RGB, FORM_GA, FORM_ZERO_ALPHA = range(5)


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_DIR, "libpixo_emu_png_reduce.so"))
        L.emu_png_convert.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.c_void_p]
        L.emu_png_index.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        L.emu_png_palette_bits.restype = L.emu_png_gray_bits.restype = C.c_uint32
        _LIB = L
    return _LIB


def convert(src, form, spp, bits, zero_alpha, w, h, row_bytes, bmap=None):
    s = np.ascontiguousarray(src, np.uint8).reshape(-1)
    m = np.ascontiguousarray(bmap if bmap is not None else np.zeros(256), np.uint8)
    out = np.empty((h, row_bytes), np.uint8)
    assert lib().emu_png_convert(s.ctypes.data, m.ctypes.data, form, spp, bits, int(zero_alpha), w, h, row_bytes, out.ctypes.data) == 0
    return out


def index(px, pixels, spp, sorted_keys):
    p = np.ascontiguousarray(px, np.uint8).reshape(-1)
    k = np.ascontiguousarray(sorted_keys, np.uint32)
    out = np.empty(pixels, np.uint8)
    assert lib().emu_png_index(p.ctypes.data, pixels, spp, k.ctypes.data, k.size, out.ctypes.data) == 0
    return out
