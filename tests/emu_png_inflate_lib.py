"""ctypes binding for tests/emu_png_inflate/libpixo_emu_png_inflate.so: the device inflate's walk (pixo_amd/csrc/png_inflate_math.h)
compiled for the host, built on demand — and the path of the stand-alone fuzz program the same Makefile builds.  Test harness only."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_png_inflate")
FUZZ = os.path.join(_DIR, "fuzz_main")
OK, FAILED, NEEDS_HOST = 0, 1, 2
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_DIR, "libpixo_emu_png_inflate.so"))
        for name in ("step_tokens", "window_bytes", "far_distance", "stored_chunk"):
            getattr(L, "emu_pngi_" + name).restype = C.c_uint32
        for name in ("length_base", "distance_base"):
            getattr(L, "emu_pngi_" + name).argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
            getattr(L, "emu_pngi_" + name).restype = C.c_uint32
        L.emu_pngi_match_source.argtypes = [C.c_uint32, C.c_uint32]
        L.emu_pngi_match_source.restype = C.c_uint32
        L.emu_pngi_code_length_order.argtypes = [C.c_uint32]
        L.emu_pngi_code_length_order.restype = C.c_uint32
        L.emu_pngi_inflate.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.emu_pngi_inflate.restype = C.c_uint32
        L.emu_pngi_build.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.emu_pngi_build.restype = C.c_uint32
        L.emu_pngi_decode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.emu_pngi_decode.restype = C.c_uint32
        L.emu_pngi_step.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
        L.emu_pngi_step.restype = C.c_uint64
        _LIB = L
    return _LIB


def constants():
    L = lib()
    return dict(step_tokens=L.emu_pngi_step_tokens(), window_bytes=L.emu_pngi_window_bytes(), far_distance=L.emu_pngi_far_distance(),
                stored_chunk=L.emu_pngi_stored_chunk())


GUARD = 64


def inflate(z: bytes, expected: int):
    """-> dict(verdict, produced, adler, turns, bound, out): `out` the expected bytes as the walk left them (0xA5 where it wrote
    nothing); the guard bytes on both sides are checked here"""
    zi = np.frombuffer(z, np.uint8)
    block = np.full(expected + 2 * GUARD, 0xA5, np.uint8)
    produced, adler, turns, bound = C.c_uint64(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    v = lib().emu_pngi_inflate(zi.ctypes.data, zi.size, block.ctypes.data + GUARD, expected, C.byref(produced), C.byref(adler), C.byref(turns),
                               C.byref(bound))
    assert (block[:GUARD] == 0xA5).all() and (block[GUARD + expected:] == 0xA5).all(), "the walk wrote outside its region"
    return dict(verdict=int(v), produced=produced.value, adler=adler.value, turns=turns.value, bound=bound.value,
                out=block[GUARD:GUARD + expected].tobytes())


def build(lengths):
    """code lengths -> the 1024-entry lookup (symbol | length << 12) as a list, or None for an over-subscribed set"""
    a = np.array(lengths, np.uint8)
    lut = np.zeros(1024, np.uint16)
    return None if lib().emu_pngi_build(a.ctypes.data, a.size, lut.ctypes.data) else lut.tolist()


def decode(lengths, bits):
    """The walk's decode of the 15 bits `bits` -> (symbol, code length), or None"""
    a = np.array(lengths, np.uint8)
    r = lib().emu_pngi_decode(a.ctypes.data, a.size, bits)
    return (r & 0xFFF, r >> 12) if r else None


def token_literal(byte):
    return 1 | (byte << 24)


def token_match(length, distance):
    return length | ((distance - 1) << 9)


def step(prefix: bytes, tokens) -> bytes:
    """One step replayed lane by lane behind `prefix`: tokens are ints (literals) and (length, distance) pairs"""
    p = np.frombuffer(prefix or b"\0", np.uint8)
    t = np.array([token_literal(x) if isinstance(x, int) else token_match(*x) for x in tokens], np.uint32)
    out = np.zeros(len(tokens) * 258 + 16, np.uint8)
    n = lib().emu_pngi_step(p.ctypes.data, len(prefix), t.ctypes.data, t.size, out.ctypes.data)
    return out[:n].tobytes()


def write_corpus(path, streams):
    """streams: [(zlib stream, expected)] in the format fuzz_main reads"""
    with open(path, "wb") as f:
        f.write(b"PIFZ" + struct.pack("<I", len(streams)))
        for z, expected in streams:
            f.write(struct.pack("<IQ", len(z), expected) + z)
