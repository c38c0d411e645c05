"""TEST HARNESS: builds tests/emu_jpeg_decode on demand and loads its shim — pixo_amd/csrc/jpeg_decode_host.cpp and
jpeg_decode_math.h compiled for the host."""
import ctypes as C
import os
import subprocess

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_jpeg_decode")
MAIN = os.path.join(DIR, "jpeg_decode_main")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(DIR, "libpixo_emu_jpeg_decode.so"))
        L.emu_jd_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t] + [C.POINTER(C.c_uint32)] * 3 + [C.c_char_p]
        L.emu_jd_within_bound.argtypes = [C.c_void_p, C.c_size_t]
        L.emu_jd_record_bytes.restype = L.emu_jd_lds_bytes.restype = C.c_uint32
        _LIB = L
    return _LIB


def decode(data, capacity, misalign=0):
    """The kernel's code over every tile of the image, the image `misalign` bytes behind a 16-byte boundary:
    (status, message, width, height, colour type, pixels)"""
    buf = np.frombuffer(bytes(data), np.uint8)
    out = np.zeros(max(capacity, 1), np.uint8)
    w, h, ct = C.c_uint32(), C.c_uint32(), C.c_uint32()
    msg = C.create_string_buffer(256)
    rc = lib().emu_jd_decode(buf.ctypes.data, buf.size, misalign, out.ctypes.data, capacity, w, h, ct, msg)
    return rc, msg.value.decode(), w.value, h.value, ct.value, out.tobytes()[:w.value * h.value * (ct.value + 1)] if rc == 0 else b""


def within_bound(data) -> int:
    buf = np.frombuffer(bytes(data), np.uint8)
    return lib().emu_jd_within_bound(buf.ctypes.data, buf.size)
