"""ctypes binding for tests/emu_png_quantize/libpixo_emu_png_quantize.so: the arithmetic of the PNG quantisation kernels
(pixo_amd/csrc/png_quantize_math.h) compiled for the host, built on demand.  Test harness only."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_png_quantize")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_DIR, "libpixo_emu_png_quantize.so"))
        L.emu_pngq_distance.argtypes = [C.c_uint32, C.c_uint32]
        L.emu_pngq_cell_color.argtypes = [C.c_uint32]
        L.emu_pngq_nearest.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.emu_pngq_distance.restype = L.emu_pngq_cell_color.restype = L.emu_pngq_nearest.restype = L.emu_pngq_dither_pixel.restype = C.c_uint32
        L.emu_pngq_dither_adjust.argtypes = [C.c_int32, C.c_int32]
        L.emu_pngq_dither_adjust.restype = C.c_int32
        L.emu_pngq_lut.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.emu_pngq_lut.restype = None
        L.emu_pngq_dither_pixel.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.emu_pngq_dither_image.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.emu_pngq_dither_image.restype = None
        _LIB = L
    return _LIB


def nearest(palette, color):
    p = np.ascontiguousarray(palette, np.uint32)
    return lib().emu_pngq_nearest(p.ctypes.data, p.size, int(color))


def lut(palette):
    p, out = np.ascontiguousarray(palette, np.uint32), np.empty(64 ** 3, np.uint8)
    lib().emu_pngq_lut(p.ctypes.data, p.size, out.ctypes.data)
    return out


def dither_pixel(table, palette, key, in16):
    p, t = np.ascontiguousarray(palette, np.uint32), np.ascontiguousarray(table, np.uint8)
    i, e = np.ascontiguousarray(in16, np.int32), np.zeros(3, np.int32)
    idx = lib().emu_pngq_dither_pixel(t.ctypes.data, p.ctypes.data, p.size, int(key), i.ctypes.data, e.ctypes.data)
    return idx, e.tolist()


def dither_image(keys, w, h, table, palette):
    k, p, t = np.ascontiguousarray(keys, np.uint32), np.ascontiguousarray(palette, np.uint32), np.ascontiguousarray(table, np.uint8)
    out = np.empty(w * h, np.uint8)
    lib().emu_pngq_dither_image(k.ctypes.data, w, h, t.ctypes.data, p.ctypes.data, p.size, out.ctypes.data)
    return out
