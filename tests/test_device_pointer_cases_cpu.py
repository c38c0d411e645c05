"""The case tables of tests/device_pointer_cases.py against the models alone: every case reaches the outcome it claims, so
that tests/test_gpu_device_pointers.py cannot pass for lack of content.  No GPU."""
import zlib

import numpy as np
import pytest

import device_pointer_cases as DP
import oracle_lib as O
import png_decode_cases as PC
import png_quantize_cases as QC
import png_reduce_model as RM


def test_offset_pairs_flip_what_they_say():
    ins, outs = {i for i, _ in DP.IN_OUT}, {o for _, o in DP.IN_OUT}
    for side in (ins, outs):
        assert {1, 2, 3} <= side                                   # every % 4 predicate false
        assert any(v % 4 == 0 and v % 16 for v in side)            # % 4 kept, % 16 lost
        assert any(v and v % 16 == 0 for v in side) and 0 in side  # every fast path, at another base and at the allocation's own
    for i in DP.REDUCE_IN_OFFSETS + DP.QUANT_IN_OFFSETS:
        assert (i, DP.OUT_FOR[i]) in DP.IN_OUT
    assert DP.PAD % 64 == 0


@pytest.mark.parametrize("c", DP.FILTER_CASES, ids=[c["name"] for c in DP.FILTER_CASES])
def test_filter_cases(c):
    w, h, bpp = c["w"], c["h"], c["bpp"]
    assert w * h > 4096, "at most 4096 pixels the adaptive strategies become Sub"
    assert (w * bpp) % 4 == c["row_mod4"]
    assert (h <= 32) == c["stateful"]  # A4 is the deliberate h = 32 exception
    if c["name"].startswith("A3"):
        limits = {4100: (16 * 1024, 32 * 1024), 8200: (32 * 1024, 48 * 1024 - 64), 12600: (48 * 1024, 1 << 31)}[w]
        assert limits[0] < w * bpp <= limits[1]
    px = DP.filter_content(w, h, bpp, 1)
    for strategy in c["strategies"]:
        if strategy in DP.ADAPTIVE:
            flt, _ = O.png_filter(px, w, h, bpp, strategy, stateful_fast=c["stateful"])
            kinds = set(flt[::w * bpp + 1].tolist())
            if c["stateful"]:
                assert len(kinds) == 1  # the first row's winner on every row
            else:
                assert len(kinds) >= 3, (strategy, kinds)


@pytest.mark.parametrize("c", DP.REDUCE_CASES, ids=[c["name"] for c in DP.REDUCE_CASES])
def test_reduce_cases(c):
    w, h, ct, spp = c["w"], c["h"], c["ct"], DP.SPP[c["ct"]]
    assert w * h > 4096 and (w * h) % 4 == DP.REDUCE_WIDTHS.index(w)
    px = DP.reduce_input(c)
    for key, outcome in c["outcomes"].items():
        stream, lay, _ = RM.prepare(px, w, h, ct, DP.reduce_model_options(key))
        got = (lay["color_type_byte"], lay["bit_depth"], lay["bytes_per_pixel"])
        if outcome in ("unchanged", "zero_alpha"):
            assert got == (RM.PNG_CT[ct], 8, spp) and not lay["palette"]
            o = DP.reduce_model_options(key)
            plain = RM.prepare(px, w, h, ct, RM.Opts(o.filter_strategy, flags=o.flags))[0]  # the filters alone
            assert np.array_equal(plain, stream) == (outcome == "unchanged"), "optimize_alpha acts exactly where claimed"
        elif outcome == "gray":
            assert got == (0, 8, 1)
        elif outcome == "gray_alpha":
            assert got == (4, 8, 2)
        elif outcome == "rgb":
            assert got == (2, 8, 3)
        else:
            assert outcome[0] == "indexed" and got == (3, outcome[1], 1)
            n = len(lay["palette"])
            assert (n <= 64) == (c["cls"] == "pal5"), "the co-occurrence counters are where the class says"


@pytest.mark.parametrize("q", DP.QUANT_CASES, ids=[q["c"]["name"] for q in DP.QUANT_CASES])
def test_quantize_cases(q):
    c = q["c"]
    palette, idx, rec = QC.model(c, q["max_colors"], q["dithering"])
    assert rec["early_out"] == q["early_out"]
    assert len(palette) <= q["max_colors"] and idx.size == c["w"] * c["h"]
    bands = (c["h"] + 63) // 64
    if q["form"] == "chained":
        assert q["dithering"] and not q["early_out"] and bands > 1
    elif q["form"] == "banded":
        assert q["dithering"] and not q["early_out"] and bands == 1
    else:
        assert q["early_out"] or not q["dithering"]
    if c["color_type"] == 3:  # an alpha read wrongly changes the result: some pixels are not opaque
        assert (QC.make_input(c).reshape(-1, 4)[:, 3] != 255).any()


@pytest.mark.parametrize("d", DP.DECODE_CASES, ids=[d["name"] for d in DP.DECODE_CASES])
def test_decode_cases(d):
    want = PC.model(d["file"])
    assert not isinstance(want, Exception), want
    w, h, pixels, ct = want
    assert (w, h) == (d["w"], d["h"]) and len(pixels) == w * h * d["out_bpp"]
    assert (w * d["out_bpp"]) % 16 == d["row_out_mod16"] and len(pixels) % 4 == d["total_mod4"]
    if "copy16" in d["path"]:
        assert d["depth"] == 8 and d["row_out_mod16"] == 0
    if "tail" in d["path"]:
        assert len(pixels) == 135 and d["total_mod4"] == 3
    stream = zlib.decompress(b"".join(DP.FC.parse(d["file"])[0]))
    assert len(stream) % h == 0 and set(stream[::len(stream) // h]) == set(range(5)), "rows cycle all five filters"


def test_zlib_cases():
    cases = DP.zlib_cases()
    assert [len(data) for _, data, _, _, _ in cases] == [1, 3, 65535, 65536, 2 * 65535 + 7, 200000]
    for name, data, bpp, row, shrinks in cases:
        assert DP.host_zlib_shrinks(data) == shrinks, name
        assert (bpp, row) == ((4, DP.ZLIB_MIXED_ROW) if shrinks else (0, 0))
    # the mixed input: stretches that deflate and stretches that do not, in turn
    mixed = cases[-1][1]
    ratios = [len(zlib.compress(mixed[at:at + 20000], 6)) / 20000 for at in range(0, len(mixed), 20000)]
    assert all(r < 0.6 for r in ratios[0::2]) and all(r >= 1.0 for r in ratios[1::2])


def test_file_cases():
    cases = DP.file_cases()
    assert sorted({c["color_type"] for c in cases}) == [0, 1, 2, 3]
    for ct in range(4):
        mine = [c for c in cases if c["color_type"] == ct]
        assert min(c["w"] * c["h"] for c in mine) == min(c["w"] * c["h"] for c in DP.FC.CASES if c["color_type"] == ct)
        assert {c["preset"] for c in mine} >= {1}
