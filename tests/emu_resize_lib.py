"""ctypes binding for tests/emu_resize/libpixo_emu_resize.so: the resize arithmetic of the device kernels
(pixo_amd/csrc/resize_math.h) compiled for the host, built on demand.  Test harness only."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_resize")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_DIR, "libpixo_emu_resize.so"))
        L.emu_resize.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
        L.emu_resize_sinf.argtypes = [C.c_float]
        L.emu_resize_sinf.restype = C.c_float
        _LIB = L
    return _LIB


def resize(data, sw, sh, dw, dh, bpp, algorithm) -> bytes:
    px = np.ascontiguousarray(data, np.uint8).reshape(-1)
    assert px.size == sw * sh * bpp
    out = np.empty(dw * dh * bpp, np.uint8)
    rc = lib().emu_resize(px.ctypes.data, sw, sh, out.ctypes.data, dw, dh, bpp, algorithm)
    assert rc == 0
    return out.tobytes()


def sinf(x: float) -> float:
    return float(lib().emu_resize_sinf(x))
