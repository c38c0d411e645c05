"""The audit of the device DEFLATE (pixo_amd/csrc/png_deflate.hip): what `png.zlib_compress` wrote is not only inflated but
read token by token (tests/deflate_tokens.py), and every stage is checked against its plain reference
(tests/deflate_reference.py) by the layers of tests/deflate_audit.py.  Layout, token validity, maximal matches, explicit
candidates, the entropy stage and the choice of form hold for ANY match finder and say what a rewrite of the finder must
keep; the last layer pins today's finder to its model.  One compression per case, shared by the layers; the inputs
(tests/deflate_cases.py) are proved to reach their edges in tests/test_deflate_tokens_cpu.py.

With PIXO_DEFLATE_AUDIT=<file> every case appends one line of figures (profiles/png_deflate_audit.txt is such a run)."""
import os

import numpy as np
import pytest

import deflate_audit as A
import deflate_cases as C
import deflate_reference as R
import deflate_tokens as T
import png_file_cases as PF
import synth

pytestmark = pytest.mark.gpu

_RUNS = {}


def png():
    from pixo_amd import png as P
    return P


def audited(name):
    """-> (stream, the stream as read, data, bpp, row), compressed and read once per case"""
    if name not in _RUNS:
        _, data, bpp, row = C.get(name)
        stream = png().zlib_compress(data, bpp=bpp, row=row)
        z = T.read_zlib(stream)
        _RUNS[name] = (stream, z, data, bpp, row)
        path = os.environ.get("PIXO_DEFLATE_AUDIT")
        if path:
            with open(path, "a") as f:
                f.write(A.record(name, z, A.chunks_of(z, data)) + "\n")
    return _RUNS[name]


def chunks(name):
    stream, z, data, bpp, row = audited(name)
    return A.chunks_of(z, data)


@pytest.mark.parametrize("name", C.NAMES)
def test_layout(name):
    stream, z, data, _, _ = audited(name)
    assert stream[:2] == b"\x78\x9c"
    A.layout(z, stream, data)


@pytest.mark.parametrize("name", C.NAMES)
def test_token_validity(name):
    A.validity(chunks(name), audited(name)[2])


@pytest.mark.parametrize("name", C.NAMES)
def test_matches_are_maximal(name):
    A.maximal(chunks(name), audited(name)[2])


@pytest.mark.parametrize("name", C.NAMES)
def test_no_explicit_candidate_is_missed(name):
    _, _, data, bpp, row = audited(name)
    A.explicit(chunks(name), data, bpp, row)


@pytest.mark.parametrize("name", C.NAMES)
def test_entropy_stage(name):
    A.entropy(chunks(name))


@pytest.mark.parametrize("name", C.NAMES)
def test_form_choice(name):
    """(A stored block shows no tokens; it is judged with the model's in test_todays_finder.)"""
    _, z, data, _, _ = audited(name)
    A.form(z, chunks(name), data)


@pytest.mark.parametrize("name", C.NAMES)
def test_todays_finder(name):
    _, z, data, bpp, row = audited(name)
    tokens, offered = C.model(name)
    cs = chunks(name)
    A.todays_finder(cs, data, bpp, row, tokens, offered)
    A.form(z, cs, data, tokens)


def test_the_row_cases_are_what_prepare_writes():
    for name in ("flat_row", "gradient_row"):
        c, px = C.row_case_input(name)
        stream, layout, _ = png().prepare(px, PF.options(c))
        assert stream.tobytes() == C.get(name)[1] and (layout.bytes_per_pixel, layout.row_bytes + 1) == C.get(name)[2:]


@pytest.mark.parametrize("name", [n for n in C.NAMES if n.startswith("window_")] + ["wide_tokens"])
def test_device_entry_gives_the_same_tokens(name):
    import torch
    stream, z, data, bpp, row = audited(name)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    cap = png().stored_bound(len(data))
    for shift in (0, 1):  # an output address that is not a multiple of 4 takes the byte path of the compaction
        d_out = torch.zeros(cap + 8, dtype=torch.uint8, device="cuda")
        n = png().zlib_compress_device(d_in, len(data), d_out[shift:], cap, bpp=bpp, row=row)
        got = T.read_zlib(d_out[shift:shift + n].cpu().numpy().tobytes())
        assert [b.tokens for b in got.blocks] == [b.tokens for b in z.blocks] and got.data == data
        assert [(b.btype, b.start, b.end) for b in got.blocks] == [(b.btype, b.start, b.end) for b in z.blocks]


def encode_hints(layout):
    """The hints png.encode gives its compressor (png_encode_api.cpp, the view png_segment_of_image leaves in its segment): the bytes of a pixel — 1 where samples are
    packed below 8 bits or are palette indices — and the bytes of a row with its filter byte, row_bytes + 1."""
    bytewise = layout.bit_depth < 8 or layout.color_type_byte == 3
    return (1 if bytewise else layout.bytes_per_pixel), layout.row_bytes + 1


def whole_file(c):
    px = PF.make_input(c)
    idat, _ = PF.parse(png().encode(px, PF.options(c)))
    prepared, layout, _ = png().prepare(px, PF.options(c))
    return b"".join(idat), prepared.tobytes(), encode_hints(layout)


@pytest.mark.parametrize("name", ["flat_row", "gradient_row", "photo_128x96_c2_p2"])
def test_encode_writes_the_tokens_of_the_model(name):
    c = C.row_case_input(name)[0] if name.endswith("_row") else next(c for c in PF.CASES if c["name"] == name)
    stream, data, (bpp, row) = whole_file(c)
    if name.endswith("_row"):
        assert (data, bpp, row) == C.get(name)[1:]
    seen = []
    tokens = R.finder_model(data, bpp, row, seen)
    A.all_layers(stream, data, bpp, row, tokens, seen)


def test_two_idat_chunks_across_the_seam():
    w = h = 300
    px = synth.rgba_noise_alpha1(w, h, 12)
    o = png().PngOptions.fast(w, h)
    idat, _ = PF.parse(png().encode(px, o))
    assert len(idat) == 2 and len(idat[0]) == PF.IDAT_BYTES
    stream = b"".join(idat)
    data = png().prepare(px, o)[0].tobytes()
    z = T.read_zlib(stream)
    cs = A.layout(z, stream, data)
    A.validity(cs, data)
    seam = 8 * PF.IDAT_BYTES
    assert any(b.start < seam < b.end for b, _, _, _ in cs), "no block lies across the IDAT seam"
