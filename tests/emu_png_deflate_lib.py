"""ctypes binding for tests/emu_png_deflate/libpixo_emu_png_deflate.so: the arithmetic of the device DEFLATE
(pixo_amd/csrc/png_deflate_math.h) compiled for the host, built on demand.  Test harness only."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_png_deflate")
_LIB = None
STORED, FIXED, DYNAMIC, SMALLEST = range(4)


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_DIR, "libpixo_emu_png_deflate.so"))
        L.emu_huffman_lengths.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.emu_kraft.argtypes = [C.c_void_p, C.c_uint32]
        L.emu_kraft.restype = C.c_uint32
        L.emu_canonical_codes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.emu_symbols.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        L.emu_crc32.argtypes = [C.c_uint32, C.c_char_p, C.c_uint64]
        L.emu_crc32.restype = C.c_uint32
        L.emu_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
        L.emu_crc32_combine.restype = C.c_uint32
        L.emu_zlib_header.argtypes = [C.c_uint32, C.c_void_p]
        L.emu_stored_bound.argtypes = [C.c_uint64]
        L.emu_stored_bound.restype = C.c_uint64
        L.emu_block.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.emu_block.restype = C.c_uint32
        _LIB = L
    return _LIB


def huffman_lengths(freq, max_bits):
    f = np.ascontiguousarray(freq, np.uint32)
    out = np.zeros(f.size, np.uint8)
    lib().emu_huffman_lengths(f.ctypes.data, f.size, max_bits, out.ctypes.data)
    return out


def kraft(lens):
    """Sum of 2^-len over the used symbols, scaled by 2^15 (a complete code: 32768)."""
    a = np.ascontiguousarray(lens, np.uint8)
    return int(lib().emu_kraft(a.ctypes.data, a.size))


def canonical_codes(lens):
    a = np.ascontiguousarray(lens, np.uint8)
    out = np.zeros(a.size, np.uint16)
    lib().emu_canonical_codes(a.ctypes.data, a.size, out.ctypes.data)
    return out


def symbols(length, dist):
    out = np.zeros(6, np.uint32)
    lib().emu_symbols(length, dist, out.ctypes.data)
    return tuple(int(v) for v in out)


def match(length, dist):
    return (length << 16) | dist


def block(tokens, data, mode, last=False):
    """-> (bytes of the block, the empty stored block behind it unless `last`; the form chosen)"""
    t = np.ascontiguousarray(tokens, np.uint32)
    out = np.zeros(len(data) + 1024, np.uint8)
    chosen = C.c_uint32()
    n = lib().emu_block(t.ctypes.data, t.size, bytes(data), len(data), mode, int(last), out.ctypes.data, C.byref(chosen))
    assert n, "the block's bits do not add up to the sizes computed for it"
    return out[:n].tobytes(), chosen.value


def crc32(data, crc=0):
    return int(lib().emu_crc32(crc, bytes(data), len(data)))


def crc32_combine(a, b, len_b):
    return int(lib().emu_crc32_combine(a, b, len_b))


def zlib_header(level):
    out = np.zeros(2, np.uint8)
    lib().emu_zlib_header(level, out.ctypes.data)
    return out.tobytes()


def stored_bound(n):
    return int(lib().emu_stored_bound(n))
