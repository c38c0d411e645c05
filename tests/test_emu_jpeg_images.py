"""CPU-only: the ragged form of the JPEG kernels on the host (pixo_amd/csrc/jpeg_images_math.h, compiled by
tests/emu_jpeg_images): the tile -> image and group -> segment searches the kernels run against a linear scan, the classes
against rules restated here, the tables of a sub-batch — first tiles, first groups, packed-stream offsets, and the planes'
places against pixo_hip_coeff_geometry — and a stand-alone program that runs the same searches under the host compiler's
address and undefined-behaviour sanitizers (a child process: nothing is loaded into python under a sanitizer)."""
import ctypes as C
import os
import random
import subprocess

import pytest

from pixo_amd import jpeg

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_jpeg_images")
_LIB = None
M420, M444, MGRAY = 0, 1, 2
BYTES, ALIGNED, FUNNEL = 0, 1, 2


class TileRecord(C.Structure):
    """pixo_jpeg_images::TileRecord"""
    _fields_ = [("px", C.c_uint64)] + [(n, C.c_uint32) for n in ("first_tile", "wh", "units", "tiles_x", "y_block", "cb_block", "cr_block", "reserved")]


class SegRecord(C.Structure):
    """pixo_jpeg_images::SegRecord"""
    _fields_ = [(n, C.c_uint32) for n in ("first_group", "blocks", "y_block", "cb_block", "cr_block", "reserved")] + [("stream_word", C.c_uint64)]


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_DIR, "libpixo_emu_jpeg_images.so"))
        u32, u64, p32, p64 = C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        L.emu_ji_image_of_tile.argtypes = [C.POINTER(TileRecord), u32, u32]
        L.emu_ji_image_of_tile.restype = u32
        L.emu_ji_segment_of_group.argtypes = [C.POINTER(SegRecord), u32, u32]
        L.emu_ji_segment_of_group.restype = u32
        L.emu_ji_shape_of.argtypes = [C.c_int, u32, u32, p32]
        L.emu_ji_shape_of.restype = None
        L.emu_ji_load_form_of.argtypes = [u64, u32, u32]
        L.emu_ji_stream_words_of.argtypes = [u32]
        L.emu_ji_stream_words_of.restype = u64
        L.emu_ji_build_tables.argtypes = [p64, u32, C.c_int, C.POINTER(TileRecord), p32, C.POINTER(SegRecord), p32, p32, C.POINTER(C.c_int), p64, p64, p64]
        assert L.emu_ji_tile_record_bytes() == C.sizeof(TileRecord) == 40 and L.emu_ji_seg_record_bytes() == C.sizeof(SegRecord) == 32
        _LIB = L
    return _LIB


def ceil_div(a, b):
    return -(-a // b)


def build(items, rgb_mode):
    """items: (address, w, h, gray) -> dict of the tables"""
    L = lib()
    n = len(items)
    flat = (C.c_uint64 * (4 * n))(*[v for it in items for v in (it[0], it[1], it[2], int(it[3]))])
    tiles, tile_item = (TileRecord * n)(), (C.c_uint32 * n)()
    segs, seg_item = (SegRecord * (n + 2))(), (C.c_uint32 * (n + 2))()
    first_group, load = (C.c_uint32 * n)(), (C.c_int * n)()
    launches, passes, counts = (C.c_uint64 * 30)(), (C.c_uint64 * 12)(), (C.c_uint64 * 5)()
    assert L.emu_ji_build_tables(flat, n, rgb_mode, tiles, tile_item, segs, seg_item, first_group, load, launches, passes, counts) == 1
    return dict(tiles=tiles, tile_item=list(tile_item[:counts[0]]), segs=segs, seg_item=list(seg_item[:counts[2]]), first_group=list(first_group), load=list(load),
                launches=[tuple(launches[5 * i:5 * i + 5]) for i in range(counts[1])], passes=[tuple(passes[6 * i:6 * i + 6]) for i in range(counts[3])],
                n_tiles=counts[0], n_segs=counts[2], blocks=counts[4])


def random_items(rng, n, max_side):
    items, at = [], rng.randrange(16)
    for _ in range(n):
        gray = rng.random() < 0.5
        w, h = rng.randint(1, max_side), rng.randint(1, max_side if rng.random() < 0.25 else 24)
        items.append((at, w, h, gray))
        at += w * h * (1 if gray else 3) + rng.randrange(5)
    return items


def test_shapes_against_the_tile_geometry_restated():
    L = lib()
    out = (C.c_uint32 * 6)()
    for mode, unit, per_tile, tile_h in ((M420, 16, 32, 16), (M444, 8, 64, 8), (MGRAY, 8, 64, 24)):
        for w, h in [(1, 1), (7, 9), (16, 16), (512, 16), (513, 17), (520, 8), (1537, 9), (1536, 24), (1537, 25), (97, 53), (65535, 3), (3, 65535)]:
            L.emu_ji_shape_of(mode, w, h, out)
            ux, uy = ceil_div(w, unit), ceil_div(h, unit)
            assert list(out) == [ux, uy, ceil_div(ux, per_tile), ceil_div(uy * unit, tile_h), 4 * ux * uy if mode == M420 else ux * uy, 0 if mode == MGRAY else ux * uy]
            ct, ss = (0, 0) if mode == MGRAY else (2, 1 if mode == M420 else 0)
            assert (out[4], out[5]) == jpeg.coefficient_geometry(w, h, ct, ss)


def test_load_forms():
    L = lib()
    for address in range(0, 9):
        for w in range(1, 14):
            for bpp in (1, 3):
                want = BYTES if w < 4 else (ALIGNED if address % 4 == 0 and (w * bpp) % 4 == 0 else FUNNEL)
                assert L.emu_ji_load_form_of(address, w, bpp) == want, (address, w, bpp)
    assert L.emu_ji_load_form_of((1 << 40) + 4, 8, 3) == ALIGNED and L.emu_ji_load_form_of((1 << 40) + 6, 8, 3) == FUNNEL


@pytest.mark.parametrize("rgb_mode", [M420, M444])
@pytest.mark.parametrize("n,max_side", [(1, 30), (1, 3000), (2, 700), (37, 700), (400, 90)])
def test_tables_and_both_searches_against_a_linear_scan(n, max_side, rgb_mode):
    L = lib()
    rng = random.Random(n * 1000 + max_side + rgb_mode)
    items = random_items(rng, n, max_side)
    t = build(items, rgb_mode)
    assert t["n_tiles"] == n and sorted(t["tile_item"]) == list(range(n))
    out = (C.c_uint32 * 6)()
    # the tuple: image after image in index order, Y then Cb then Cr, as pixo_hip_coeff_geometry counts them
    at, y_at = 0, []
    for (_, w, h, gray) in items:
        yb, cb = jpeg.coefficient_geometry(w, h, 0 if gray else 2, 1 if rgb_mode == M420 else 0)
        y_at.append((at, at + yb, at + yb + cb, yb + 2 * cb))
        at += yb + 2 * cb
    assert t["blocks"] == at
    seen_classes = []
    for mode, load, first, count, tiles in t["launches"]:
        seen_classes.append((mode, load))
        table = (TileRecord * count)(*t["tiles"][first:first + count])  # (exactly the launch's records)
        tile, last_item = 0, -1
        for r in range(count):
            k = t["tile_item"][first + r]
            addr, w, h, gray = items[k]
            assert k > last_item, "index order inside a class"
            last_item = k
            assert (mode == MGRAY) == gray and t["load"][k] == load == L.emu_ji_load_form_of(addr, w, 1 if gray else 3)
            L.emu_ji_shape_of(mode, w, h, out)
            rec = table[r]
            assert (rec.px, rec.first_tile, rec.wh, rec.units, rec.tiles_x) == (addr, tile, w | h << 16, out[0] | out[1] << 16, out[2])
            assert (rec.y_block, rec.cb_block, rec.cr_block) == y_at[k][:3]
            n_tiles = out[2] * out[3]
            for probe in {tile, tile + n_tiles - 1, tile + rng.randrange(n_tiles)}:  # its first, its last, one in between
                assert L.emu_ji_image_of_tile(table, count, probe) == r
            tile += n_tiles
        assert tile == tiles
    assert seen_classes == sorted(seen_classes, key=lambda c: (c[0] != MGRAY, c[1])) and len(set(seen_classes)) == len(seen_classes)
    for mode, first, count, groups, blocks, words in t["passes"]:
        table = (SegRecord * (count + 1))(*t["segs"][first:first + count + 1])
        group, word, total = 0, 0, 0
        for r in range(count):
            k = t["seg_item"][first + r]
            rec = table[r]
            assert (mode == MGRAY) == items[k][3]
            assert (rec.first_group, rec.blocks, rec.stream_word) == (group, y_at[k][3], word) and t["first_group"][k] == group
            assert (rec.y_block, rec.cb_block, rec.cr_block) == y_at[k][:3]
            g = ceil_div(rec.blocks, 192)
            for probe in {group, group + g - 1, group + rng.randrange(g)}:
                assert L.emu_ji_segment_of_group(table, count, probe) == r
            group += g
            word += L.emu_ji_stream_words_of(rec.blocks)
            total += rec.blocks
            assert L.emu_ji_stream_words_of(rec.blocks) * 4 >= rec.blocks * 209 + 64 and L.emu_ji_stream_words_of(rec.blocks) % 4 == 0
        assert (group, total, word) == (groups, blocks, words) and table[count].first_group == groups and t["seg_item"][first + count] == 0xFFFFFFFF
    assert sum(p[2] for p in t["passes"]) == n


def test_the_searches_on_tables_of_1_2_and_65535_entries():
    L = lib()
    for count in (1, 2, 65535):
        tiles, segs = (TileRecord * count)(), (SegRecord * (count + 1))()
        sizes = [1 + (i * 7) % 5 if i % 3 else 1 for i in range(count)]
        at = 0
        for i, s in enumerate(sizes):
            tiles[i].first_tile = segs[i].first_group = at
            at += s
        segs[count].first_group = at
        probes = range(at) if count < 100 else list(range(0, 200)) + list(range(at - 200, at)) + list(range(0, at, 997))
        want, i = {}, 0
        for p in range(at):  # the linear scan
            while i + 1 < count and tiles[i + 1].first_tile <= p:
                i += 1
            want[p] = i
        for p in probes:
            assert L.emu_ji_image_of_tile(tiles, count, p) == want[p] and L.emu_ji_segment_of_group(segs, count, p) == want[p], (count, p)


def test_the_search_program_under_sanitizers():
    lib()  # (builds it)
    r = subprocess.run([os.path.join(_DIR, "search_main"), "12"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "search_main ok" in r.stdout
    print(r.stdout.strip())
