"""ctypes binding for tests/emu_png_batch/libpixo_emu_png_batch.so: the segment arithmetic of the PNG batch kernels
(pixo_amd/csrc/png_deflate_math.h) compiled for the host, built on demand.  Test harness only."""
import ctypes as C
import os
import subprocess

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_png_batch")
_LIB = None
CHUNK, WINDOW, IDAT, PIECE, ALIGN = 65535, 32768, 256 * 1024, 4096, 16


class Segment(C.Structure):
    """pixo_pngz::ZSegment"""
    _fields_ = [("src", C.c_uint64), ("len", C.c_uint64), ("dst", C.c_uint64), ("first_chunk", C.c_uint32), ("first_piece", C.c_uint32),
                ("hint_bpp", C.c_uint32), ("hint_row", C.c_uint32), ("adler", C.c_uint32), ("reserved", C.c_uint32)]


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_DIR, "libpixo_emu_png_batch.so"))
        L.emu_seg_layout.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(Segment)]
        for name in ("emu_seg_of_chunk", "emu_seg_of_piece"):
            getattr(L, name).argtypes = [C.POINTER(Segment), C.c_uint32, C.c_uint32]
            getattr(L, name).restype = C.c_uint32
        L.emu_chunk_span.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
        L.emu_chunk_span.restype = None
        L.emu_piece_span.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
        L.emu_piece_span.restype = C.c_uint32
        for name in ("emu_seg_chunks", "emu_seg_pieces", "emu_seg_dst_bytes", "emu_seg_framed_size", "emu_seg_framed_offset", "emu_stored_bound"):
            getattr(L, name).argtypes = [C.c_uint64]
            getattr(L, name).restype = C.c_uint64
        assert L.emu_segment_bytes() == C.sizeof(Segment)
        _LIB = L
    return _LIB


def layout(lens):
    """-> the table of len(lens) + 1 segments"""
    n = len(lens)
    table = (Segment * (n + 1))()
    assert lib().emu_seg_layout((C.c_uint64 * n)(*lens), n, table) == 1
    return table


def chunk_span(length, chunk):
    out = (C.c_uint64 * 4)()
    lib().emu_chunk_span(length, chunk, out)
    return int(out[0]), int(out[1]), int(out[2]), bool(out[3])  # c0, wstart, n, last


def piece_span(stream_len, piece):
    s0 = C.c_uint64()
    n = lib().emu_piece_span(stream_len, piece, C.byref(s0))
    return int(s0.value), int(n)
