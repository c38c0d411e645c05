"""CPU-only: the colour conversion's host-and-device header on the host (pixo_amd/csrc/convert_math.h, compiled by
tests/emu_convert): the tile -> image search the kernels run against a linear walk, that the workgroups of a launch together
write every output byte of every image exactly once (also with the tiles of an image capped, through the stride loop), the
table of a sub-batch against the driver's plan, the luma over all 2^24 Rgb triples and the 16-pixel step against the numpy
model, the whole lane body over host memory against the model, and a stand-alone program that runs the same code over
buffers of exactly the images' bytes under the host compiler's address and undefined-behaviour sanitizers (a child process:
nothing is loaded into python under a sanitizer)."""
import ctypes as C
import random
import subprocess

import numpy as np
import pytest

import convert_cases as CC
import convert_model as M
import emu_convert_lib as E
from pixo_amd import convert

MAX_TILES = (1 << 31) - 1


def test_constants_and_kinds_match_the_library_and_the_model():
    L = E.lib()
    assert L.emu_cv_tile_pixels() == convert.tile_pixels() and L.emu_cv_image_tiles() == 65536
    for s in range(5):
        for d in range(5):
            want = M.kind_of(s, d) if s < 4 and d < 4 else None
            assert L.emu_cv_kind_of(s, d) == (-1 if want is None else want), (s, d)
    for ct in range(4):
        assert L.emu_cv_target_type(0, ct) == M.target_type(M.OPAQUE, ct) and L.emu_cv_target_type(1, ct) == M.target_type(M.TO_GRAY, ct)
    assert L.emu_cv_target_type(2, 0) == -1
    T = L.emu_cv_tile_pixels()
    for pixels, cap, want in [(1, 65536, 1), (T, 65536, 1), (T + 1, 65536, 2), (5 * T, 2, 2), (5 * T, 1, 1), (1 << 48, 65536, 65536), (65536 * T, 65536, 65536),
                              (65535 * T + 1, 65536, 65536), (65535 * T, 65536, 65535)]:
        assert L.emu_cv_tiles_of(pixels, cap) == want, (pixels, cap)


def _table(count, cap, seed):
    """`count` images of one class with seeded sizes -> (records, launch)"""
    T = convert.tile_pixels()
    rnd = random.Random(seed)
    items = [(0, 0, rnd.choice([1, 17, T - 1, T, T + 1, 3 * T + 5, 5 * T]) if count < 1000 else 1 + i % 3, M.K_RGBA_RGB, 4) for i in range(count)]
    table, launches, order = E.build_table(items, cap, MAX_TILES)
    assert len(launches) == 1 and order == list(range(count))
    return table, launches[0], items


@pytest.mark.parametrize("count", (1, 2, 3, 64, 65, 65535))
def test_every_tile_finds_the_image_a_linear_walk_gives(count):
    L = E.lib()
    for cap in (65536, 2):
        table, launch, items = _table(count, cap, 700 + count)
        want = [i for i in range(count) for _ in range(L.emu_cv_tiles_of(items[i][2], cap))]
        assert launch.tiles == len(want) and launch.count == count
        assert [table[i].first_tile for i in range(count)] == [want.index(i) for i in range(count)] if count < 100 else True
        tiles = range(launch.tiles) if launch.tiles < 5000 else list(range(0, launch.tiles, 97)) + [launch.tiles - 1]
        for t in tiles:
            assert L.emu_cv_image_of_tile(table, count, t) == want[t], (count, cap, t)


@pytest.mark.parametrize("cap", (65536, 3, 2, 1))
def test_the_tiles_of_an_image_cover_each_output_byte_exactly_once(cap):
    L = E.lib()
    T = convert.tile_pixels()
    sizes = [1, 15, 16, 17, T - 1, T, T + 1, 64 * 65, 5 * T, 5 * T + 9]
    for dbpp in (1, 3, 4):
        at, items = 0, []
        for p in sizes:
            items.append((0, at, p, M.K_COPY, dbpp))
            at += p * dbpp + 5  # (a gap nobody may touch)
        table, launches, _ = E.build_table(items, cap, MAX_TILES)
        assert 1 <= len(launches) <= 2  # (the offsets make some images aligned, some not)
        hits = np.zeros(at, np.uint32)
        for l in launches:
            records = C.cast(C.byref(table, l.first_record * C.sizeof(E.Record)), C.POINTER(E.Record))
            assert L.emu_cv_cover(records, l.count, l.tiles, dbpp, hits.ctypes.data_as(C.POINTER(C.c_uint32)), at) == 0
        want = np.zeros(at, np.uint32)
        for (_, o, p, _, _) in items:
            want[o:o + p * dbpp] = 1
        assert np.array_equal(hits, want), (cap, dbpp)


def test_the_table_matches_the_drivers_plan():
    """The same images through the plan entry (kinds, forms, tiles, launches) and through build_table"""
    T = convert.tile_pixels()
    rnd = random.Random(710)
    for cap, switch in ((65536, None), (2, b"convert_images_tiles=2")):
        shapes = [(rnd.choice([1, 17, T, T + 1, 64]), rnd.choice([1, 3, 5]), rnd.randrange(4)) for _ in range(40)]
        src, _ = CC.block_of(shapes, 0, odd={i for i in range(40) if i % 3 == 0})
        dst, _ = convert.layout_images(src, convert.Target.OPAQUE if cap == 2 else convert.Target.GRAY)
        from pixo_amd import _lib
        try:
            _lib.load().pixo_hip_debug_configure(switch)
            plan = convert.convert_images_plan(src, dst, 0, 0)
        finally:
            _lib.load().pixo_hip_debug_configure(None)
        launches_total = 0
        for a, b in zip(plan["sub_first"], plan["sub_first"][1:]):
            items = [(s[3], d[3], s[0] * s[1], M.kind_of(int(s[2]), int(d[2])), int(s[2]) + 1) for s, d in zip(src[a:b], dst[a:b])]
            built = E.build_table(items, cap, 2 * cap if switch else MAX_TILES)
            assert built is not None, "the plan's sub-batch does not fit a launch"
            table, launches, order = built
            launches_total += len(launches)
            for r, k in enumerate(order):
                i = a + k
                assert table[r].tiles == plan["tiles"][i] and table[r].pixels == src[i][0] * src[i][1]
            for l in launches:
                members = order[l.first_record:l.first_record + l.count]
                assert members == sorted(members)  # index order inside a class
                assert {(plan["kind"][a + k], plan["form"][a + k]) for k in members} == {(l.cls // 2, l.cls % 2)}
                assert l.tiles == sum(plan["tiles"][a + k] for k in members)
            assert [l.cls for l in launches] == sorted({l.cls for l in launches})
        assert launches_total == plan["launches"]
    assert E.build_table([(0, 0, 5 * T, M.K_COPY, 1)] * 3, 2, 4) is None and E.build_table([(0, 0, 5 * T, M.K_COPY, 1)] * 2, 2, 4) is not None


def test_the_luma_over_all_rgb_triples():
    out = np.empty(1 << 24, np.uint8)
    E.lib().emu_cv_luma_all(out.ctypes.data)
    assert np.array_equal(out, M.convert(CC.all_triples(), M.RGB, M.GRAY))


def test_the_16_pixel_step_over_random_groups():
    L = E.lib()
    groups = 4099
    for kind, (s_ct, d_ct) in M.PAIRS.items():
        px = CC.pixels(16 * groups, 1, s_ct, 720 + kind)
        px[:16 * M.bpp(s_ct)] = 255  # (and the extremes)
        px[16 * M.bpp(s_ct):32 * M.bpp(s_ct)] = 0
        out = np.empty(16 * groups * M.bpp(d_ct), np.uint8)
        L.emu_cv_convert16(kind, px.ctypes.data, out.ctypes.data, groups)
        assert np.array_equal(out, M.convert(px, s_ct, d_ct)), kind


@pytest.mark.parametrize("cap", (65536, 2))
def test_the_lane_body_over_host_memory(cap):
    """Every workgroup and lane of the launches of a mixed batch, run on the host over one block: the model's bytes, gaps untouched"""
    L = E.lib()
    T = convert.tile_pixels()
    sizes = [(1, 1), (15, 1), (16, 1), (17, 1), (5, 3), (1, 65), (T - 1, 1), (T, 1), (T + 1, 1), (64, 65), (T, 5), (T + 3, 5)]
    shapes = [(w, h, s) for w, h in sizes for s, _ in CC.ALL_PAIRS[:4]] + [(33, 7, ct) for ct in range(4)]
    dst_cts = [d for _ in sizes for _, d in CC.ALL_PAIRS[:4]] + list(range(4))
    odd = {i for i in range(len(shapes)) if i % 3 == 1}
    src, block = CC.block_of(shapes, 730, odd=odd)
    dst, total = CC.destinations(src, dst_cts, odd={i for i in range(len(shapes)) if i % 5 == 2})
    base = np.zeros(block.size + 16, np.uint8)
    s0 = (-base.ctypes.data) % 16
    base[s0:s0 + block.size] = block
    out = np.full(total + 16, CC.AFTER, np.uint8)
    d0 = (-out.ctypes.data) % 16
    items = [(base.ctypes.data + s0 + s[3], out.ctypes.data + d0 + d[3], s[0] * s[1], M.kind_of(s[2], d[2]), s[2] + 1) for s, d in zip(src, dst)]
    table, launches, _ = E.build_table(items, cap, MAX_TILES)
    assert len(launches) == 10
    for l in launches:
        assert L.emu_cv_run_launch(C.cast(C.byref(table, l.first_record * C.sizeof(E.Record)), C.POINTER(E.Record)), l.count, l.tiles, l.cls // 2, l.cls % 2) == 0
    assert np.all(out[:d0] == CC.AFTER) and np.all(out[d0 + total:] == CC.AFTER)
    CC.check_block(out[d0:d0 + total], block, src, dst)


def test_the_program_under_sanitizers():
    E.lib()  # (builds it)
    r = subprocess.run([E.MAIN, "24"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "convert_main ok" in r.stdout
    print(r.stdout.strip())
