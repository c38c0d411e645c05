"""The generator's small cases (tests/random_cases.py) through the emulated device code (tests/emu: the kernels' tile code
compiled for the host), against the oracle: the coefficient kernel in its packed and scalar forms with all three load forms
(`misalign` puts the rows off a dword boundary, widths below 4 take the byte gathers), and the PNG filter's group arithmetic."""
import ctypes as C

import numpy as np
import pytest

import emu_lib as E
import oracle_lib as O
import random_cases as R

SEEDS = (932, 955, 20261016)


def _small_jpeg(seed, n, limit=30000):
    return [d for d in R.cases(seed, n) if d["kind"] == "jpeg" and d["ct"] in (0, 2) and d["w"] * d["h"] * (d.get("batch") or 1) <= limit]


@pytest.mark.parametrize("seed", SEEDS)
def test_emulated_coefficients_on_random_cases(seed):
    for d in _small_jpeg(seed, 120):
        px = R.image(d)
        want = O.coeffs(px, d["w"], d["h"], d["ct"], d["ss"], d["q"])
        for misalign in sorted({0, d.get("offset", 0) % 4 or 1}):
            got = E.coeffs(px, d["w"], d["h"], d["ct"], d["ss"], d["q"], misalign=misalign)  # (packed and scalar forms both)
            for g, w, plane in zip(got[:3], want, ("Y", "Cb", "Cr")):
                assert np.array_equal(g, w), "%s differs, misalign %d: %s" % (plane, misalign, R.replay_line(d))


def _emu_png(px, w, h, bpp, strategy):
    L = E.lib()
    L.emu_png_filter.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p]
    L.emu_png_filter.restype = C.c_long
    out = np.zeros(h * (w * bpp + 1), np.uint8)
    ad = L.emu_png_filter(px.ctypes.data, w, h, bpp, strategy, out.ctypes.data)
    return out, ad & 0xFFFFFFFF


@pytest.mark.parametrize("seed", SEEDS)
def test_emulated_png_groups_on_random_cases(seed):
    n = 0
    for d in R.cases(seed, 400):
        if d["kind"] != "png" or d["w"] * d["h"] * d["bpp"] > 300000:
            continue
        if d["strategy"] >= 6 and (d["w"] * d["h"] <= 4096 or d["h"] <= 32):
            continue  # the launcher's host rules (Sub for small images, the sequential fast form): tested on the C ABI
        want, wad = O.png_filter(R.image(d), d["w"], d["h"], d["bpp"], d["strategy"], stateful_fast=False)
        got, gad = _emu_png(R.image(d), d["w"], d["h"], d["bpp"], d["strategy"])
        assert np.array_equal(got, want) and gad == wad, R.replay_line(d)
        n += 1
    assert n >= 10
