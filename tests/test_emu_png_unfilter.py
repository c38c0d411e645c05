"""The PNG decoder's arithmetic header (pixo_amd/csrc/png_unfilter_math.h) on the host against the model
(tests/png_decode_model.py): the five filters at every filter unit, the Paeth ties, wrap-around, every depth's unpacking at
ragged widths, and the palette rules."""
import zlib

import pytest

import emu_png_unfilter_lib as E
import png_decode_cases as PC
import png_decode_model as M
import synth


@pytest.mark.parametrize("bpp", [1, 2, 3, 4, 6, 8])
@pytest.mark.parametrize("ft", [0, 1, 2, 3, 4])
def test_every_filter_at_every_filter_unit(ft, bpp):
    h, rb = 5, 7 * bpp + 0
    stream = bytearray(synth.lcg_bytes(h * (rb + 1), 10 * ft + bpp).tobytes())
    for y in range(h):
        stream[y * (rb + 1)] = ft
    rows, bad = E.unfilter(bytes(stream), h, rb, bpp)
    assert bad == -1 and rows == M.reconstruct(bytes(stream), h, rb, bpp)


def test_filter_units_and_row_bytes():
    L = E.lib()
    for ct, d in PC.COMBOS:
        assert L.emu_pngu_filter_unit(ct, d) == M.filter_unit(ct, d)
        for w in (1, 7, 8, 9, 1000):
            assert L.emu_pngu_row_bytes(ct, d, w) == M.row_bytes(ct, d, w)


def test_paeth_ties_resolve_a_then_b_then_c():
    L = E.lib()
    assert L.emu_pngu_paeth(7, 7, 7) == 7          # a = b = c
    assert L.emu_pngu_paeth(10, 10, 12) == 10       # pa = pb < pc: a
    assert L.emu_pngu_paeth(11, 8, 10) == 8         # pb = pc < pa: b
    for a in range(0, 256, 5):
        for b in range(0, 256, 7):
            for c in range(0, 256, 11):
                assert L.emu_pngu_paeth(a, b, c) == M.paeth(a, b, c)


def test_sums_wrap_and_average_floors():
    L = E.lib()
    assert L.emu_pngu_reconstruct(1, 1, 255, 0, 0) == 0            # 255 + 1
    assert L.emu_pngu_reconstruct(2, 200, 0, 100, 0) == 44
    assert L.emu_pngu_reconstruct(3, 0, 255, 255, 0) == 255        # the 9-bit sum 510, halved
    assert L.emu_pngu_reconstruct(3, 7, 0, 5, 0) == 9              # floor(5 / 2)
    assert L.emu_pngu_reconstruct(4, 250, 10, 20, 10) == (250 + 20) & 255
    assert L.emu_pngu_reconstruct(0, 9, 1, 2, 3) == 9


def test_a_filter_byte_above_4_is_reported_by_row():
    stream = bytes([0, 1, 2, 5, 3, 4, 9, 5, 6])
    assert E.unfilter(stream, 3, 2, 1)[1] == 1


@pytest.mark.parametrize("w", [1, 7, 8, 9])
@pytest.mark.parametrize("ct,depth", PC.COMBOS)
def test_unpacking_and_conversion_of_every_depth(ct, depth, w):
    h = 3
    png = PC.make(w, h, ct, depth, seed=w + depth, trns=PC.trns_for(ct, depth, w))
    f = M.walk(png)
    rb = M.row_bytes(ct, depth, w)
    rows, _ = E.unfilter(zlib.decompress(f["idat"]), h, rb, M.filter_unit(ct, depth))
    assert E.convert(rows, w, h, ct, depth, f["plte"], f["trns"]) == PC.model(png)[2]


def test_palette_rules():
    w, h = 9, 2
    for depth in (1, 2, 4, 8):
        # an index beyond PLTE: black, opaque when the output is RGBA
        for trns in (None, bytes([0]), bytes([255, 255])):
            png = PC.make(w, h, 3, depth, seed=5, plte_entries=1, trns=trns)
            f = M.walk(png)
            rows, _ = E.unfilter(zlib.decompress(f["idat"]), h, M.row_bytes(3, depth, w), 1)
            want = PC.model(png)
            got = E.convert(rows, w, h, 3, depth, f["plte"], f["trns"])
            assert got == want[2]
            assert len(got) == w * h * (4 if trns == bytes([0]) else 3)  # tRNS all 255: RGB out
            if trns == bytes([0]):
                assert b"\0\0\0\xff" in got  # beyond the palette
    # tRNS shorter than PLTE: entries beyond it are opaque
    png = PC.make(8, 1, 3, 8, filters=0, seed=9, trns=bytes([7, 8]))
    f = M.walk(png)
    rows, _ = E.unfilter(zlib.decompress(f["idat"]), 1, 8, 1)
    got = E.convert(rows, 8, 1, 3, 8, f["plte"], f["trns"])
    assert got == PC.model(png)[2]
    assert all(got[4 * x + 3] == ({0: 7, 1: 8}.get(rows[x], 255)) for x in range(8))
