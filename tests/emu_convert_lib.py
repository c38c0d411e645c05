"""TEST HARNESS: builds tests/emu_convert on demand and loads its shim — pixo_amd/csrc/convert_math.h compiled for the host."""
import ctypes as C
import os
import subprocess

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_convert")
MAIN = os.path.join(DIR, "convert_main")
_LIB = None


class Record(C.Structure):
    """pixo_convert::Record"""
    _fields_ = [(n, C.c_uint64) for n in ("src", "dst", "pixels")] + [(n, C.c_uint32) for n in ("first_tile", "tiles", "bpp", "reserved")]


class Item(C.Structure):
    """pixo_convert::Item"""
    _fields_ = [(n, C.c_uint64) for n in ("src", "dst", "pixels")] + [(n, C.c_uint32) for n in ("kind", "bpp")]


class Launch(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("cls", "first_record", "count", "tiles")]


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(DIR, "libpixo_emu_convert.so"))
        u32, u64, p32, p8 = C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_void_p
        L.emu_cv_kind_of.argtypes = [u32, u32]
        L.emu_cv_target_type.argtypes = [u32, u32]
        L.emu_cv_image_of_tile.argtypes = [C.POINTER(Record), u32, u32]
        L.emu_cv_image_of_tile.restype = u32
        L.emu_cv_tiles_of.argtypes = [u64, u32]
        L.emu_cv_tiles_of.restype = u32
        L.emu_cv_build_table.argtypes = [C.POINTER(Item), u32, u32, u64, C.POINTER(Record), C.POINTER(Launch), p32]
        L.emu_cv_luma_all.argtypes = [p8]
        L.emu_cv_luma_all.restype = None
        L.emu_cv_convert16.argtypes = [C.c_int, p8, p8, u32]
        L.emu_cv_convert16.restype = None
        L.emu_cv_run_launch.argtypes = [C.POINTER(Record), u32, u32, C.c_int, C.c_int]
        L.emu_cv_cover.argtypes = [C.POINTER(Record), u32, u32, u32, p32, u64]
        for name in ("emu_cv_record_bytes", "emu_cv_item_bytes", "emu_cv_tile_pixels", "emu_cv_image_tiles"):
            getattr(L, name).restype = u32
        assert L.emu_cv_record_bytes() == C.sizeof(Record) == 40 and L.emu_cv_item_bytes() == C.sizeof(Item) == 32
        _LIB = L
    return _LIB


def build_table(items, image_tiles, launch_tiles):
    """items: (src, dst, pixels, kind, bpp) -> (records, launches, record_item), or None when the builder refuses"""
    L = lib()
    n = len(items)
    arr = (Item * max(n, 1))(*[Item(*it) for it in items])
    table, launches, order = (Record * max(n, 1))(), (Launch * max(n, 1))(), (C.c_uint32 * max(n, 1))()
    k = L.emu_cv_build_table(arr, n, image_tiles, launch_tiles, table, launches, order)
    if k < 0:
        return None
    return table, list(launches[:k]), list(order[:n])
