"""CPU-only: the ragged form of the PNG filter kernels on the host (pixo_amd/csrc/png_images_math.h, compiled by
tests/emu_png_images): the row -> image search the kernel runs against a linear walk, the records' src, dst and sums_at
against the driver's layout worked out here, and the launch class of an image against launch_bpp's conditions restated here."""
import ctypes as C
import os
import random
import subprocess

import pytest

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_png_images")
_LIB = None

GENERAL, REGS, BIGRAMS, REGS512, BIGRAMS_REGS = 0, 1, 2, 3, 4
S_PAETH, S_MINSUM, S_ADAPTIVE, S_ADAPTIVE_FAST, S_BIGRAMS = 4, 5, 6, 7, 8


class Record(C.Structure):
    """pixo_png_images::Record"""
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("sums_at", C.c_uint64), ("row_bytes", C.c_uint32), ("height", C.c_uint32),
                ("first_row", C.c_uint32), ("strategy", C.c_int32)]


class Item(C.Structure):
    """pixo_png_images::Item"""
    _fields_ = [("image", C.c_uint32), ("src", C.c_uint64), ("dst", C.c_uint64), ("row_bytes", C.c_uint32), ("height", C.c_uint32),
                ("bpp", C.c_uint32), ("strategy", C.c_int32)]


class Launch(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("cls", "bpp", "kind", "fast", "staged", "first_record", "count", "rows", "max_row_bytes")]


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_DIR, "libpixo_emu_png_images.so"))
        L.emu_image_of_row.argtypes = [C.POINTER(Record), C.c_uint32, C.c_uint32]
        L.emu_image_of_row.restype = C.c_uint32
        L.emu_kind_of.argtypes = [C.c_int, C.c_uint64]
        L.emu_stage_bytes.argtypes = [C.c_uint64]
        L.emu_stage_bytes.restype = C.c_uint32
        L.emu_class_of.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int]
        L.emu_class_of.restype = C.c_uint32
        L.emu_fast_of.argtypes = [C.c_uint64, C.c_uint64]
        L.emu_build_table.argtypes = [C.POINTER(Item), C.c_uint32, C.c_uint64, C.POINTER(Record), C.POINTER(Launch), C.POINTER(C.c_uint32)]
        assert L.emu_record_bytes() == C.sizeof(Record) == 40 and L.emu_item_bytes() == C.sizeof(Item)
        _LIB = L
    return _LIB


def table_of_heights(heights):
    t = (Record * len(heights))()
    at = 0
    for i, h in enumerate(heights):
        t[i].height, t[i].first_row = h, at
        at += h
    return t, at


def height_lists():
    rng = random.Random(20262)
    lists = [[1], [7], [1, 1], [1] * 33, [3, 1, 1, 5, 1], [2048], [1, 4000, 1]]
    for _ in range(8):
        lists.append([rng.choice([1, 1, 2, rng.randint(1, 40), rng.randint(100, 700)]) for _ in range(rng.randint(1, 70))])
    return lists


HEIGHTS = height_lists()


@pytest.mark.parametrize("heights", HEIGHTS, ids=["list%d" % i for i in range(len(HEIGHTS))])
def test_every_launch_row_finds_the_image_and_row_a_linear_walk_gives(heights):
    L = lib()
    t, rows = table_of_heights(heights)
    y = 0
    for image, h in enumerate(heights):  # the walk: image after image, row after row
        for line in range(h):
            got = L.emu_image_of_row(t, len(heights), y)
            assert (got, y - t[got].first_row) == (image, line), y
            y += 1
    assert y == rows


def stage_bytes(row_bytes):
    """launch_png_filter_rows: 16 bytes in front, the row in whole 16-byte groups, 32 bytes of slack; nothing beyond 48 KiB"""
    stage = 16 + ((row_bytes + 15) & ~15) + 32
    return stage if stage <= 48 * 1024 else 0


def kind_restated(strategy, row_bytes):
    """launch_bpp's conditions (kRegIters 4, kThreads 256: 4096 dwords in the registers of 256 threads, 8192 of 512)"""
    ndw = (row_bytes + 3) // 4
    staged = stage_bytes(row_bytes) != 0
    if strategy == S_BIGRAMS and staged and ndw <= 4 * 256 * 4:
        return BIGRAMS_REGS
    if strategy == S_BIGRAMS:
        return BIGRAMS
    if strategy > S_PAETH and ndw <= 4 * 2 * 256 * 4 and staged:
        return REGS if ndw <= 4 * 256 * 4 else REGS512
    return GENERAL


ROWS = [1, 3, 4, 5, 16380, 16381, 16384, 16385, 16388, 32764, 32765, 32768, 32769, 49087, 49088, 49089, 49104, 49105, 49200, 1 << 26]


def test_class_choice_is_launch_bpps():
    L = lib()
    for row_bytes in ROWS:
        assert L.emu_stage_bytes(row_bytes) == stage_bytes(row_bytes), row_bytes
        for strategy in range(9):
            assert L.emu_kind_of(strategy, row_bytes) == kind_restated(strategy, row_bytes), (strategy, row_bytes)
    # the edges in words: the last row 256 threads hold, the first of 512, the last of 512, the last the stage holds
    assert [kind_restated(S_ADAPTIVE, n) for n in (16384, 16385, 32768, 32769)] == [REGS, REGS512, REGS512, GENERAL]
    assert [kind_restated(S_BIGRAMS, n) for n in (16384, 16385)] == [BIGRAMS_REGS, BIGRAMS]
    assert stage_bytes(49104) == 49152 and stage_bytes(49105) == 0
    assert [kind_restated(s, 100) for s in range(5)] == [GENERAL] * 5
    for address, row_bytes in [(0, 4), (4, 8), (1, 4), (2, 4), (0, 6), (16, 3), (3, 3)]:
        assert L.emu_fast_of(address, row_bytes) == int(address % 4 == 0 and row_bytes % 4 == 0)
    keys = {L.emu_class_of(bpp, fast, kind, staged) for bpp in (1, 2, 3, 4) for fast in (0, 1) for kind in range(5) for staged in (0, 1)}
    assert len(keys) == 80  # one key per class


def random_items(rng, n):
    items, at = [], 0
    for image in range(n):
        bpp = rng.choice([1, 2, 3, 4])
        width = rng.choice([1, 2, 5, 64, 1000, 4096, 4097, 8193, 12300])
        height = rng.choice([1, 1, 2, 9, 40])
        strategy = rng.choice(list(range(9)))
        src = rng.randrange(0, 1 << 20)
        items.append(dict(image=2 * image + 1, src=src, dst=at, row_bytes=width * bpp, height=height, bpp=bpp, strategy=strategy))
        at += height * (width * bpp + 1) + rng.choice([0, 0, 17])  # (the driver: the unreduced streams; other images' lie between)
    return items


@pytest.mark.parametrize("seed,n,address", [(1, 1, 0), (2, 2, 1), (3, 40, 0), (4, 40, 7), (5, 200, 16), (6, 9, 2)])
def test_table_matches_the_drivers_layout(seed, n, address):
    L = lib()
    items = random_items(random.Random(seed), n)
    arr = (Item * n)(*[Item(**it) for it in items])
    table, launches, record_item = (Record * n)(), (Launch * n)(), (C.c_uint32 * n)()
    count = L.emu_build_table(arr, n, address, table, launches, record_item)
    assert count >= 1
    # sums_at: the heights of the items in front, in INDEX order whatever the class
    sums_at = [sum(it["height"] for it in items[:k]) for k in range(n)]
    assert sorted(record_item) == list(range(n))  # every item once
    want_class = []
    for k, it in enumerate(items):
        fast = int((address + it["src"]) % 4 == 0 and it["row_bytes"] % 4 == 0)
        want_class.append(L.emu_class_of(it["bpp"], fast, kind_restated(it["strategy"], it["row_bytes"]), int(stage_bytes(it["row_bytes"]) != 0)))
    assert sorted(set(want_class)) == [launches[i].cls for i in range(count)]  # one launch per class present, ascending
    at = 0
    for i in range(count):
        l = launches[i]
        assert l.first_record == at and l.count >= 1
        members = [k for k in range(n) if want_class[k] == l.cls]  # index order inside a class
        assert [record_item[at + j] for j in range(l.count)] == members
        first_row = 0
        for j, k in enumerate(members):
            r, it = table[at + j], items[k]
            assert (r.src, r.dst, r.sums_at, r.row_bytes, r.height, r.strategy) == \
                (it["src"], it["dst"], sums_at[k], it["row_bytes"], it["height"], it["strategy"])
            assert r.first_row == first_row
            assert (l.bpp, l.kind) == (it["bpp"], kind_restated(it["strategy"], it["row_bytes"]))
            assert l.staged == int(stage_bytes(it["row_bytes"]) != 0)
            first_row += it["height"]
        assert l.rows == first_row and l.max_row_bytes == max(items[k]["row_bytes"] for k in members)
        # the launch's rows find their records through the kernel's search
        sub = (Record * l.count)(*[table[at + j] for j in range(l.count)])
        for y in (0, l.rows - 1, l.rows // 2):
            got = L.emu_image_of_row(sub, l.count, y)
            assert sub[got].first_row <= y < sub[got].first_row + sub[got].height
        at += l.count
    assert at == n


def test_a_launch_of_more_than_2_31_rows_is_refused():
    L = lib()
    n = 129
    arr = (Item * n)(*[Item(image=i, src=0, dst=0, row_bytes=4, height=1 << 24, bpp=4, strategy=0) for i in range(n)])
    table, launches, record_item = (Record * n)(), (Launch * n)(), (C.c_uint32 * n)()
    assert L.emu_build_table(arr, n, 0, table, launches, record_item) == -1
    assert L.emu_build_table(arr, 127, 0, table, launches, record_item) == 1
