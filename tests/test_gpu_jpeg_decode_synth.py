"""JPEG decode on the device, on the files no encoder writes (tests/jpeg_decode_cases.py SYNTH: table assignments, component
ids, segment orders, long codes, ZRL, blocks without an end, restarts with fill bytes, odd file ends — libjpeg-turbo's pixels
committed) and on the arithmetic cases written at test time (tests/jpeg_decode_arith.py: the IDCT at the edge of its region,
scaled tables, the colour conversion over its input space, the upsamplers over a lattice of neighbour values), whose
expectations the CPU tests hold against a live Pillow.  Everything byte for byte."""
import numpy as np
import pytest

import jpeg_decode_arith as AR
import jpeg_decode_cases as JC

pytestmark = pytest.mark.gpu


def D():
    from pixo_amd import decode
    return decode


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def differs(got, want):
    """'' when the two uint8 arrays are equal"""
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    return "%d of %d bytes differ, first at byte %d: got %d, expected %d" % (bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]) if bad.size else ""


@pytest.mark.parametrize("c", JC.SYNTH, ids=JC.SYNTH_IDS)
def test_single_entries_give_the_committed_pixels(c):
    """libjpeg-turbo's pixels — the model's where Pillow refuses the file (an entry with "pillow": a table that uses the all-ones
    code word, a file without EOI), which this library decodes"""
    from pixo_amd import ColorType
    d = D()
    im = d.decode_jpeg(JC.data(c))
    assert (im.width, im.height, im.color_type) == (c["w"], c["h"], ColorType(c["color_type"]))
    assert JC.mismatch(im.pixels, c) == ""
    t, ct = d.decode_jpeg_device(JC.data(c))
    assert tuple(t.shape) == (c["h"], c["w"], c["color_type"] + 1) and ct == ColorType(c["color_type"])
    assert JC.mismatch(host(t).tobytes(), c) == ""


def test_one_batch_mixes_them_with_ordinary_files():
    """Records with three different quantisation tables beside records with two and one, in one call"""
    d = D()
    cases = [c for pair in zip(JC.SYNTH, JC.small()) for c in pair] + JC.SYNTH[len(JC.small()):]
    assert len(cases) >= len(JC.SYNTH) + 20
    views = d.decode_jpeg_batch_device([JC.data(c) for c in cases])
    for c, (t, _) in zip(cases, views):
        assert JC.mismatch(host(t).tobytes(), c) == ""


@pytest.mark.parametrize("q", [1, 4])
def test_idct_basis_sweep_and_dense_blocks(q):
    d = D()
    data, want, _ = AR.idct_sweep(q)
    assert differs(np.frombuffer(d.decode_jpeg(data).pixels, np.uint8).reshape(want.shape), want) == ""
    assert differs(host(d.decode_jpeg_device(data)[0])[..., 0], want) == ""


@pytest.mark.parametrize("name", AR.SCALED)
def test_scaled_tables(name):
    """Times 2 and 4: libjpeg's pixels.  Times 16: the clamped samples (the model's), where libjpeg's masked table wraps"""
    d = D()
    for factor in (2, 4, 16):
        data, want = AR.scaled(name, factor)
        got = host(d.decode_jpeg_device(data)[0])
        assert differs(got.reshape(want.shape), want) == "", factor


@pytest.mark.parametrize("name", AR.COLOUR_IMAGES)
def test_colour_conversion_over_its_input_space(name):
    """2048 x 2048, a block per pair of values: one pixel of every block, and ten seeded blocks whole"""
    d = D()
    data, want = AR.colour_image(name)
    t, _ = d.decode_jpeg_device(data)
    assert tuple(t.shape) == (2048, 2048, 3)
    rng = np.random.default_rng(sum(name.encode()))
    oy, ox = (int(v) for v in rng.integers(0, 8, 2))
    assert differs(host(t[oy::8, ox::8].contiguous()), want) == ""
    for by, bx in rng.integers(0, 256, (10, 2)):
        block = host(t[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].contiguous())
        assert differs(block, np.broadcast_to(want[by, bx], (8, 8, 3))) == "", (by, bx)


@pytest.mark.parametrize("mode,trim", [("422", 1), ("422", 2), ("420", 1), ("420", 2)])
def test_upsamplers_over_the_lattice_of_neighbour_values(mode, trim):
    d = D()
    data, want = AR.upsampler_image(mode, trim)
    t, _ = d.decode_jpeg_device(data)
    assert differs(host(t), want) == ""
