"""The single colour-conversion entries on the GPU (pixo_hip_convert_device / pixo_hip_convert, pixo_amd/csrc/convert.hip):
all five kinds — the copy at all four bytes-per-pixel values — byte for byte against the numpy model (tests/convert_model.py),
at sizes around the 16-pixel group and the tile, at every pairing of source and destination alignment that selects the
aligned form, the aligned form's pixelwise tail and the byte form, with the bytes in front of and behind every destination
checked to be untouched; the stride loop under the debug switch; and every Rgb triple."""
import numpy as np
import pytest

import convert_cases as CC
import convert_model as M

pytestmark = pytest.mark.gpu
PAD = 32  # bytes of sentinels in front of and behind a destination


def T():
    from pixo_amd import convert
    return convert.tile_pixels()


def run(px, w, h, s_ct, d_ct, s_off=0, d_off=0):
    """The source at s_off and the destination at d_off modulo 16 in fresh device buffers -> the destination's bytes, after the
    sentinels around it have been checked"""
    import torch
    from pixo_amd import convert
    n_out = w * h * M.bpp(d_ct)
    d_src = torch.empty(px.size + 32, dtype=torch.uint8, device="cuda")
    assert d_src.data_ptr() % 16 == 0
    d_src[s_off:s_off + px.size] = torch.from_numpy(px).cuda()
    host = np.full(PAD + 16 + n_out + PAD, CC.BEFORE, np.uint8)
    at = PAD + d_off
    host[at + n_out:] = CC.AFTER
    d_dst = torch.from_numpy(host).cuda()
    assert d_dst.data_ptr() % 16 == 0 and PAD % 16 == 0
    convert.convert_device(d_src[s_off:], w, h, s_ct, d_ct, d_dst[at:])
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.all(got[:at] == CC.BEFORE), "bytes in front of the destination were written"
    assert np.all(got[at + n_out:] == CC.AFTER), "bytes behind the destination were written"
    return got[at:at + n_out]


def shapes():
    t = T()
    return [(1, 1), (15, 1), (16, 1), (17, 1), (5, 3), (1, 65), (t - 1, 1), (t, 1), (t + 1, 1), (64, 65)]


@pytest.mark.parametrize("pair", CC.ALL_PAIRS, ids=lambda p: "%dto%d" % p)
def test_every_kind_at_every_shape(pair):
    s_ct, d_ct = pair
    for i, (w, h) in enumerate(shapes()):
        px = CC.pixels(w, h, s_ct, 100 + i)
        want = M.convert(px, s_ct, d_ct)
        assert np.array_equal(run(px, w, h, s_ct, d_ct), want), (w, h, "aligned")
        assert np.array_equal(run(px, w, h, s_ct, d_ct, 1, 3), want), (w, h, "bytes")


@pytest.mark.parametrize("pair", CC.ALL_PAIRS, ids=lambda p: "%dto%d" % p)
def test_every_alignment_of_source_and_destination(pair):
    s_ct, d_ct = pair
    for w in (17, T() + 1):
        px = CC.pixels(w, 1, s_ct, 200)
        want = M.convert(px, s_ct, d_ct)
        for s_off in (0, 1, 2, 3, 5, 16):
            for d_off in (0, 1, 2, 3):
                assert np.array_equal(run(px, w, 1, s_ct, d_ct, s_off, d_off), want), (w, s_off, d_off)


def test_the_host_entry_and_the_front_end_names():
    from pixo_amd import ColorType, convert
    w, h = 37, 29
    for s_ct, d_ct in CC.ALL_PAIRS:
        px = CC.pixels(w, h, s_ct, 300)
        assert convert.convert(px, w, h, s_ct, d_ct) == M.convert(px, s_ct, d_ct).tobytes()
    rgba, ga = CC.pixels(w, h, M.RGBA, 301), CC.pixels(w, h, M.GRAY_ALPHA, 302)
    assert convert.rgba_to_rgb(rgba.tobytes()) == M.convert(rgba, M.RGBA, M.RGB).tobytes()
    assert convert.gray_alpha_to_gray(ga) == M.convert(ga, M.GRAY_ALPHA, M.GRAY).tobytes()
    for ct in range(4):
        px = CC.pixels(w, h, ct, 303)
        assert convert.to_grayscale(px, ColorType(ct)) == M.convert(px, ct, M.GRAY).tobytes()


def test_the_stride_loop_under_the_debug_switch():
    """A 5-tile image over 2 workgroups: workgroup 0 takes tiles 0, 2 and 4, workgroup 1 tiles 1 and 3"""
    from pixo_amd import _lib
    L = _lib.load()
    w, h = T() + 7, 5  # 5 tiles and a tail
    assert (w * h + T() - 1) // T() == 6 or T() != 4096
    try:
        L.pixo_hip_debug_configure(b"convert_images_tiles=2")
        for s_ct, d_ct in CC.ALL_PAIRS:
            for w_, h_ in ((T(), 5), (w, h)):
                px = CC.pixels(w_, h_, s_ct, 400)
                want = M.convert(px, s_ct, d_ct)
                assert np.array_equal(run(px, w_, h_, s_ct, d_ct), want), (s_ct, d_ct, "aligned")
                assert np.array_equal(run(px, w_, h_, s_ct, d_ct, 3, 0), want), (s_ct, d_ct, "bytes")
    finally:
        L.pixo_hip_debug_configure(None)


def test_every_rgb_triple_to_gray():
    px = CC.all_triples()
    got = run(px, 4096, 4096, M.RGB, M.GRAY)
    want = M.convert(px, M.RGB, M.GRAY)
    assert np.array_equal(got, want), "first difference at triple %d" % int(np.flatnonzero(got != want)[0])
