"""The model of the PNG lossy mode (tests/png_quantize_model.py) against the reference's own wasm build: for every vector of
tests/golden/png_quantize_cases.json it reproduces the gate's verdict, PLTE, tRNS and every index (through the inflated
IDAT's length and sha256, and byte for byte where the reference's file is stored).  No GPU."""
import hashlib
import zlib

import pytest

import png_quantize_cases as QC
import png_quantize_model as M


@pytest.mark.parametrize("c", QC.CASES, ids=[c["name"] for c in QC.CASES])
def test_gate_verdict(c):
    spp = QC.BPP[c["color_type"]]
    keys = M.keys_of(QC.make_input(c), spp) if spp >= 3 else None
    assert M.should_quantize(M.AUTO, spp, keys, 256) == c["applied"]
    ihdr = bytes.fromhex(c["chunks"][0][1])
    indexed = ihdr[8:10] == b"\x08\x03" and c["stream_len"] == c["h"] * (c["w"] + 1)
    if c["applied"]:
        assert indexed
    elif ihdr[9] == 3:  # a lossless palette (reduce_palette): its tRNS is never trimmed and it has at most 256 of the image's own colours
        assert len(bytes.fromhex(c["chunks"][1][1])) // 3 <= 256


@pytest.mark.parametrize("c", QC.APPLIED, ids=[c["name"] for c in QC.APPLIED])
def test_model_reproduces_reference_file(c):
    palette, idx, _ = QC.model(c)
    assert [[t, b.hex()] for t, b in M.chunks_of(palette, c["w"], c["h"])] == c["chunks"]
    stream = M.indexed_stream(idx, c["w"], c["h"], 0)  # every filter byte 0: Adaptive / AdaptiveFast / Bigrams become None
    assert len(stream) == c["stream_len"] and hashlib.sha256(stream).hexdigest() == c["stream_sha256"]
    assert zlib.adler32(stream) == c["adler32"]
    if c.get("stored"):
        import png_file_cases as PF
        idat, _ = PF.parse(QC.stored_file(c))
        assert zlib.decompress(b"".join(idat)) == stream


def test_histogram_strides_of_the_large_cases():
    for name, gate_stride, hist_stride in (("pal_n4000_317x317_c2_p1", 5, 2), ("pal_n1000_512x512_c3_p0", 13, 5)):
        c = next(c for c in QC.CASES if c["name"] == name)
        n = c["w"] * c["h"]
        assert (max(n // 20000, 1), max(n // 50000, 1)) == (gate_stride, hist_stride)


def test_integer_dither_step_equals_the_f32_form():
    """The claim the integer form rests on, checked over every value the accumulators can hold: (c + E/16).clamp(0, 255) as u8
    in f32 equals t < 0 ? 0 : min(t >> 4, 255) with t = 16 c + E."""
    import numpy as np
    c = np.arange(256, dtype=np.int64)[:, None]
    e = np.arange(-16 * 255, 16 * 255 + 1, dtype=np.int64)[None, :]
    f = np.clip(c.astype(np.float32) + e.astype(np.float32) / np.float32(16), np.float32(0), np.float32(255)).astype(np.uint8)
    t = 16 * c + e
    assert np.array_equal(f, np.where(t < 0, 0, np.minimum(t >> 4, 255)).astype(np.uint8))
