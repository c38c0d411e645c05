"""ctypes binding for tests/emu_png_deflate_effort/libpixo_emu_png_deflate_effort.so: the links, chains and lazy rule of the
device DEFLATE's high effort (pixo_amd/csrc/png_deflate_math.h) compiled for the host, built on demand.  Test harness only."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_png_deflate_effort")
_LIB = None
CHUNK, WINDOW = 65535, 32768


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_DIR, "libpixo_emu_png_deflate_effort.so"))
        L.emu_effort_links.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]
        L.emu_effort_links.restype = C.c_uint32
        L.emu_effort_tokens.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.emu_effort_tokens.restype = C.c_uint32
        for name in ("emu_chain_link", "emu_chain_step", "emu_kept_length"):
            getattr(L, name).argtypes = [C.c_uint32, C.c_uint32]
            getattr(L, name).restype = C.c_uint32
        L.emu_lazy_next.argtypes = [C.c_uint32] * 3
        L.emu_lazy_next.restype = C.c_uint32
        _LIB = L
    return _LIB


def links(data, chunk, substep):
    """-> the 16-bit links of a chunk's window and of the chunk, counted from the window's start"""
    prev = np.zeros(WINDOW + 65536, np.uint16)
    n = lib().emu_effort_links(bytes(data), len(data), chunk, substep, prev.ctypes.data)
    return prev[:n]


def tokens(data, bpp, row, substep, probes):
    """-> one token list per chunk, in the form of deflate_tokens: (position, length, distance) or (position, literal)"""
    data = bytes(data)
    out = []
    for chunk in range(-(-len(data) // CHUNK)):
        tok, at = np.zeros(65536, np.uint32), np.zeros(65536, np.uint32)
        n = lib().emu_effort_tokens(data, len(data), chunk, bpp, row, substep, probes, tok.ctypes.data, at.ctypes.data)
        c0 = chunk * CHUNK
        out.append([(c0 + int(p), int(t) >> 16, int(t) & 0xFFFF) if t >> 16 else (c0 + int(p), int(t)) for t, p in zip(tok[:n], at[:n])])
    return out
