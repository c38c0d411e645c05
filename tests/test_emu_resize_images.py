"""CPU-only: the ragged form of the resize kernels on the host (pixo_amd/csrc/resize_images_math.h, compiled by
tests/emu_resize_images): the tile -> (image, tile x, tile y) search the kernels run against a linear walk, the tiles per pass
against the counts restated here, the table of a sub-batch against the driver's layout, and — the bodies' index arithmetic
walked over counters — that the workgroups of a launch together write every output element of every image exactly once,
also with an image's rows of tiles capped at 1 and 2."""
import ctypes as C
import os
import random
import subprocess

import pytest

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_resize_images")
_LIB = None
POINT, H, V = 0, 1, 2
PASSES = (POINT, H, V)
CAP = 65535
MAX_TILES = (1 << 31) - 1


class Record(C.Structure):
    """pixo_resize_images::Record"""
    _fields_ = [(n, C.c_uint64) for n in ("src", "dst", "mid_at", "mid_stride", "h_at", "v_at")] + \
        [(n, C.c_uint32) for n in ("sw", "sh", "dw", "dh", "bpp", "use_lds", "first_tile", "tiles_x", "tiles_y", "reserved")]


class Item(C.Structure):
    """pixo_resize_images::Item"""
    _fields_ = [(n, C.c_uint64) for n in ("src", "dst", "mid_at", "mid_stride", "h_at", "v_at")] + \
        [(n, C.c_uint32) for n in ("sw", "sh", "dw", "dh", "bpp", "use_lds")]


class Launch(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("bpp", "first_record", "count", "tiles")]


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_DIR, "libpixo_emu_resize_images.so"))
        u32, u64, p32 = C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)
        L.emu_image_of_tile.argtypes = [C.POINTER(Record), u32, u32]
        L.emu_image_of_tile.restype = u32
        L.emu_tile_in_image.argtypes = [u32, u32, u32, p32, p32]
        L.emu_tile_in_image.restype = None
        L.emu_tiles_of.argtypes = [C.c_int, u32, u32, u32, u32, u32, p32, p32]
        L.emu_tiles_of.restype = None
        L.emu_tile_count.argtypes = [C.c_int, u32, u32, u32, u32, u32]
        L.emu_tile_count.restype = u64
        L.emu_build_table.argtypes = [C.POINTER(Item), u32, C.c_int, u32, C.POINTER(Record), C.POINTER(Launch), p32]
        L.emu_cover.argtypes = [C.POINTER(Record), u32, u32, C.c_int, p32, u64]
        assert L.emu_record_bytes() == C.sizeof(Record) == 88 and L.emu_item_bytes() == C.sizeof(Item) == 72
        _LIB = L
    return _LIB


def ceil_div(a, b):
    return -(-a // b)


def tiles_restated(kind, sh, dw, dh, bpp, cap=CAP):
    """A point tile is 256 columns x 4 rows of the destination, a horizontal one 64 destination columns x 4 SOURCE rows, a
    vertical one 1024 bytes x 1 row of the destination; at most `cap` rows of tiles, and no more than 2^31 - 1 tiles in all"""
    across, rows = {POINT: (ceil_div(dw, 256), ceil_div(dh, 4)), H: (ceil_div(dw, 64), ceil_div(sh, 4)), V: (ceil_div(dw * bpp, 1024), dh)}[kind]
    rows = min(rows, cap, MAX_TILES // across)
    return across, rows


def tiles_of(kind, sh, dw, dh, bpp, cap=CAP):
    tx, ty = C.c_uint32(), C.c_uint32()
    lib().emu_tiles_of(kind, sh, dw, dh, bpp, cap, C.byref(tx), C.byref(ty))
    return tx.value, ty.value


M = 1 << 24
SHAPES = [(1, 1, 1), (23, 17, 13), (41, 64, 41), (300, 3, 3), (5, 257, 5), (41, 65, 9), (7, 300, 6), (2, 64, 2), (4, 256, 4), (5, 257, 5), (8, 64, 8),
          (9, 1024, 1), (3, 1025, 3), (262147, 3, 262150), (M, M, M), (M, 1, M), (1, M, 1), (262140, M, 262140), (M - 1, M - 1, M - 1)]


def test_tiles_per_pass():
    L = lib()
    for sh, dw, dh in SHAPES:
        for bpp in (1, 2, 3, 4):
            for kind in PASSES:
                for cap in (CAP, 1, 2, 7):
                    want = tiles_restated(kind, sh, dw, dh, bpp, cap)
                    assert tiles_of(kind, sh, dw, dh, bpp, cap) == want, (kind, sh, dw, dh, bpp, cap)
                    assert L.emu_tile_count(kind, sh, dw, dh, bpp, cap) == want[0] * want[1] <= MAX_TILES
    # in words: 257 columns are two point tiles, 65 two horizontal ones, 300 RGBA pixels two vertical ones; 5 rows two rows of point tiles
    assert tiles_of(POINT, 9, 257, 5, 3) == (2, 2) and tiles_of(H, 9, 65, 5, 3) == (2, 3) and tiles_of(V, 9, 300, 6, 4) == (2, 6)
    assert tiles_of(V, 9, 256, 6, 4) == (1, 6) and tiles_of(V, 9, 257, 6, 4) == (2, 6) and tiles_of(V, 9, 1024, 6, 1) == (1, 6)
    # the cap, and an image whose tiles alone would not fit one launch
    assert tiles_of(POINT, 1, 1, 4 * CAP + 1, 1) == (1, CAP) and tiles_of(H, 4 * CAP + 1, 1, 1, 1) == (1, CAP) and tiles_of(V, 1, 1, CAP + 1, 1) == (1, CAP)
    assert tiles_of(POINT, 1, M, M, 4) == (65536, 32767) and tiles_of(H, M, M, 1, 4) == (1 << 18, 8191) and tiles_of(V, 1, M, M, 4) == (65536, 32767)


def table_of_counts(counts):
    """records of (tiles_x, tiles_y), back to back"""
    t = (Record * len(counts))()
    at = 0
    for i, (tx, ty) in enumerate(counts):
        t[i].tiles_x, t[i].tiles_y, t[i].first_tile = tx, ty, at
        at += tx * ty
    return t, at


def count_lists():
    rng = random.Random(20263)
    lists = [[(1, 1)], [(3, 5)], [(1, 1), (1, 1)], [(1, 1)] * 33, [(2, 3), (1, 1), (1, 1), (5, 1), (1, 7)], [(64, 40)], [(1, 1), (50, 80), (1, 1)]]
    for _ in range(8):
        lists.append([(rng.choice([1, 1, 2, rng.randint(1, 9)]), rng.choice([1, 1, 3, rng.randint(1, 60)])) for _ in range(rng.randint(1, 70))])
    return lists


COUNTS = count_lists()


@pytest.mark.parametrize("counts", COUNTS, ids=["list%d" % i for i in range(len(COUNTS))])
def test_every_tile_finds_the_image_and_coordinates_a_linear_walk_gives(counts):
    L = lib()
    t, tiles = table_of_counts(counts)
    tx, ty = C.c_uint32(), C.c_uint32()
    tile = 0
    for image, (nx, ny) in enumerate(counts):  # the walk: image after image, row of tiles after row of tiles
        for y in range(ny):
            for x in range(nx):
                got = L.emu_image_of_tile(t, len(counts), tile)
                L.emu_tile_in_image(tile, t[got].first_tile, t[got].tiles_x, C.byref(tx), C.byref(ty))
                assert (got, tx.value, ty.value) == (image, x, y), tile
                tile += 1
    assert tile == tiles


def test_search_at_the_count_limits():
    L = lib()
    # the first and the last tile of a launch of 2^31 - 1 tiles; images of one tile beside one of nearly all
    t, tiles = table_of_counts([(1, 1), (65536, 32767), (1, 65534)])
    assert tiles == MAX_TILES
    assert [L.emu_image_of_tile(t, 3, x) for x in (0, 1, 2, 65536 * 32767, 65536 * 32767 + 1, MAX_TILES - 1)] == [0, 1, 1, 1, 2, 2]
    tx, ty = C.c_uint32(), C.c_uint32()
    L.emu_tile_in_image(65536 * 32767, 1, 65536, C.byref(tx), C.byref(ty))
    assert (tx.value, ty.value) == (65535, 32766)
    # a table of one record, of one tile and of many
    for counts in ([(1, 1)], [(7, 9)]):
        t, tiles = table_of_counts(counts)
        assert [L.emu_image_of_tile(t, 1, x) for x in range(tiles)] == [0] * tiles
    # 65535 images of one tile: every tile is its image
    t, tiles = table_of_counts([(1, 1)] * 65535)
    assert tiles == 65535 and all(L.emu_image_of_tile(t, 65535, x) == x for x in (0, 1, 2, 32767, 32768, 65533, 65534))


def random_items(rng, n, small=False):
    items = []
    for i in range(n):
        bpp = rng.choice([1, 2, 3, 4])
        pick = (lambda: rng.choice([1, 2, 3, 5, 9, 64, 65, 70])) if small else (lambda: rng.choice([1, 2, 5, 63, 64, 65, 255, 256, 257, 300, 1025, 5000]))
        sw, sh, dw, dh = pick(), pick(), pick(), pick()
        items.append(dict(src=rng.randrange(1 << 40), dst=rng.randrange(1 << 40), mid_at=16 * rng.randrange(1 << 20), mid_stride=(dw * bpp + 15) // 16 * 16,
                          h_at=16 * rng.randrange(1 << 16), v_at=16 * rng.randrange(1 << 16), sw=sw, sh=sh, dw=dw, dh=dh, bpp=bpp, use_lds=rng.randrange(2)))
    return items


def build(items, kind, cap=CAP):
    n = len(items)
    arr = (Item * n)(*[Item(**it) for it in items])
    table, launches, record_item = (Record * n)(), (Launch * n)(), (C.c_uint32 * n)()
    count = lib().emu_build_table(arr, n, kind, cap, table, launches, record_item)
    return count, table, launches, list(record_item)


@pytest.mark.parametrize("seed,n", [(1, 1), (2, 2), (3, 40), (4, 41), (5, 200), (6, 9)])
def test_table_matches_the_drivers_layout(seed, n):
    L = lib()
    items = random_items(random.Random(seed), n)
    for kind in PASSES:
        for cap in (CAP, 1, 2):
            count, table, launches, record_item = build(items, kind, cap)
            assert sorted(record_item) == list(range(n))  # every item once
            groups = [0] if kind == V else sorted({it["bpp"] for it in items})  # the vertical pass is byte-wise: one launch
            assert [launches[i].bpp for i in range(count)] == groups
            at = 0
            for i in range(count):
                l = launches[i]
                members = [k for k in range(n) if kind == V or items[k]["bpp"] == l.bpp]  # index order inside a launch
                assert l.first_record == at and l.count == len(members) and record_item[at:at + l.count] == members
                first_tile = 0
                for j, k in enumerate(members):
                    r, it = table[at + j], items[k]
                    assert {f: getattr(r, f) for f in it} == it
                    assert (r.tiles_x, r.tiles_y) == tiles_restated(kind, it["sh"], it["dw"], it["dh"], it["bpp"], cap)
                    assert r.first_tile == first_tile and r.reserved == 0
                    first_tile += r.tiles_x * r.tiles_y
                assert l.tiles == first_tile
                # the launch's tiles find their records through the kernel's search
                sub = (Record * l.count)(*[table[at + j] for j in range(l.count)])
                for tile in (0, l.tiles - 1, l.tiles // 2):
                    got = L.emu_image_of_tile(sub, l.count, tile)
                    assert sub[got].first_tile <= tile < sub[got].first_tile + sub[got].tiles_x * sub[got].tiles_y
                at += l.count
            assert at == n


def test_a_launch_of_more_than_2_31_tiles_is_refused():
    big = dict(src=0, dst=0, mid_at=0, mid_stride=0, h_at=0, v_at=0, sw=2, sh=2, dw=M, dh=4 * 16384, bpp=4, use_lds=0)  # 65536 x 16384 = 2^30 point tiles
    one = dict(big, dw=2, dh=2)
    assert build([big], POINT)[0] == 1
    count, _, launches, _ = build([big, dict(big, dh=4 * 16383), dict(one, dh=4 * 65535)], POINT)
    assert count == 1 and launches[0].tiles == MAX_TILES  # 2^30 + (2^30 - 65536) + 65535
    assert build([big, dict(big, dh=4 * 16383), dict(one, dh=4 * 65535), one], POINT)[0] == -1
    assert build([big, big], POINT)[0] == -1
    assert build([big, dict(big, bpp=3)], POINT)[0] == 2  # launches of their own
    assert build([big, dict(big, bpp=3)], V)[0] == -1  # 65536 x 32767 and 49152 x 43690 tiles in the one vertical launch


# ---- coverage: the bodies' loops over counters -------------------------------------------------------------------------------
def cover(items, kind, cap):
    """-> per item, the counters of its output elements after every workgroup of every launch of the pass has run"""
    L = lib()
    sizes = [(it["sh"] * it["dw"] if kind == H else it["dw"] * it["dh"] * (it["bpp"] if kind == V else 1)) for it in items]
    starts, at = [], 0
    for s in sizes:
        starts.append(at)
        at += s + 3  # (a gap that nothing may touch)
    placed = [dict(it, dst=starts[i]) for i, it in enumerate(items)]
    count, table, launches, _ = build(placed, kind, cap)
    assert count >= 1
    hits = (C.c_uint32 * at)()
    for i in range(count):
        l = launches[i]
        sub = (Record * l.count)(*[table[l.first_record + j] for j in range(l.count)])
        assert L.emu_cover(sub, l.count, l.tiles, kind, hits, at) == 0
    hits = list(hits)
    return [hits[s:s + n] for s, n in zip(starts, sizes)], [hits[s + n:s + n + 3] for s, n in zip(starts, sizes)]


RAGGED_SRC = [(37, 23), (64, 41), (1, 1), (5, 300), (300, 5), (64, 41), (129, 7), (2200, 2)]
RAGGED_DST = [(17, 13), (64, 41), (1, 1), (3, 3), (257, 5), (65, 9), (300, 6), (64, 2)]


def ragged_items(rotation):
    return [dict(src=0, dst=0, mid_at=0, mid_stride=0, h_at=0, v_at=0, sw=sw, sh=sh, dw=dw, dh=dh, bpp=(i + rotation) % 4 + 1, use_lds=1)
            for i, ((sw, sh), (dw, dh)) in enumerate(zip(RAGGED_SRC, RAGGED_DST))]


@pytest.mark.parametrize("cap", (CAP, 1, 2, 3))
@pytest.mark.parametrize("kind", PASSES)
def test_all_tiles_of_an_image_cover_each_output_element_exactly_once(kind, cap):
    sets = [ragged_items(r) for r in range(4)] + [random_items(random.Random(77 + cap), 25, small=True),
                                                  [dict(ragged_items(0)[0], sh=1100, dw=700, dh=1100, bpp=3)]]
    for items in sets:
        inside, gaps = cover(items, kind, cap)
        for i, (cells, gap) in enumerate(zip(inside, gaps)):
            assert set(cells) == {1}, "pass %d, cap %d, image %d: an element written %s times" % (kind, cap, i, sorted(set(cells)))
            assert gap == [0, 0, 0], "pass %d, cap %d: bytes behind image %d were written" % (kind, cap, i)
