"""PNG decode through the C ABI without a GPU: pixo_hip_png_decode_info on every case, every refusal of the walk with the
model's exact string and status (and the order of two faults), and the host inflate (pixo_hip_zlib_inflate) against
zlib.decompress and against every error string of the reference's inflate (src/decode/inflate.rs, bit_reader.rs) that a
stream can reach.  Two of the reference's strings cannot be reached by any stream and are not raised here: "code length too
large" (lengths come from 4-bit symbols) and "invalid code length code" (the code-length table has 19 symbols)."""
import struct
import zlib

import numpy as np
import pytest

import deflate_cases  # noqa: F401  (kept importable: the encoder's cases live beside these)
import png_decode_cases as PC
import png_decode_model as M
import png_file_cases as FC
from pixo_amd import ColorType, decode, error

GOOD = list(PC.shape_cases(64)) + list(PC.layout_cases())
BROKEN = list(PC.broken_cases())
CLASS = {M.INVALID_DIMENSIONS: error.InvalidDimensions, M.IMAGE_TOO_LARGE: error.ImageTooLarge, M.INVALID_DECODE: error.InvalidDecode,
         M.UNSUPPORTED_DECODE: error.UnsupportedDecode}


def test_info_on_every_case():
    for name, png in GOOD:
        w, h, _, ct = PC.model(png)
        assert decode.decode_png_info(png) == (w, h, ColorType(ct)), name


@pytest.mark.parametrize("name,png", BROKEN, ids=[n for n, _ in BROKEN])
def test_refusals_match_the_model(name, png):
    want = PC.model(png)
    assert isinstance(want, M.DecodeError)
    with pytest.raises(error.Error) as e:
        decode.decode_png_info(png)
    assert str(e.value) == str(want) and type(e.value) is CLASS[want.status]
    with pytest.raises(error.Error) as e:  # the decoding entry refuses it the same way, before it needs a GPU
        decode.decode_png(png)
    assert str(e.value) == str(want) and type(e.value) is CLASS[want.status]


# ---- the host inflate -------------------------------------------------------------------------------------------------------
class BitsOut:
    """LSB-first bit writer for crafted DEFLATE streams"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, v, n):  # a Huffman code: most significant bit first
        for i in range(n - 1, -1, -1):
            self.bits((v >> i) & 1, 1)
        return self

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def zwrap(body, data=b"", adler=None):
    return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(data) if adler is None else adler)


def stored(data, final=True):
    return bytes([1 if final else 0]) + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data


def fixed_lit(b, v):  # the fixed literal/length code of symbol v
    if v < 144:
        return b.code(0x30 + v, 8)
    if v < 256:
        return b.code(0x190 + v - 144, 9)
    if v < 280:
        return b.code(v - 256, 7)
    return b.code(0xC0 + v - 280, 8)


def lcg(n, seed):
    import synth
    return synth.lcg_bytes(n, seed).tobytes()


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def inflate_ok(z, data):
    assert decode.inflate_zlib(z, len(data)) == data


def test_inflate_stored_fixed_dynamic_and_several_blocks():
    text = (b"the quick brown fox jumps over the lazy dog. " * 40) + lcg(3000, 1)
    inflate_ok(zwrap(stored(text), text), text)
    inflate_ok(zwrap(raw_deflate(text, 6, zlib.Z_FIXED), text), text)
    inflate_ok(zlib.compress(text, 9), text)
    inflate_ok(zwrap(stored(text[:100], False) + raw_deflate(text[100:]), text), text)
    big = lcg(70000, 2) + bytes(70000) + lcg(200000, 3)[::2] * 2  # long enough for several dynamic blocks
    c = zlib.compressobj(6)
    z = c.compress(big[:100000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(big[100000:]) + c.flush()
    inflate_ok(z, big)
    inflate_ok(zlib.compress(b"", 6), b"")
    inflate_ok(zlib.compress(b"a", 6), b"a")


def test_inflate_longest_match_and_farthest_distance():
    far = lcg(32768, 4) + lcg(32768, 4)[:300]  # matches at distance 32768
    z = zlib.compress(far, 9)
    inflate_ok(z, far)
    b = BitsOut().bits(1, 1).bits(1, 2)  # by hand: literal, then length 258 at distance 1; then 32768 literals and distance 32768
    fixed_lit(b, 65)
    fixed_lit(b, 285).code(0, 5)
    fixed_lit(b, 256)
    inflate_ok(zwrap(b.done(), b"A" * 259), b"A" * 259)
    head = lcg(32768, 5)
    b = BitsOut().bits(1, 1).bits(1, 2)
    for v in head:
        fixed_lit(b, v)
    fixed_lit(b, 285).code(29, 5).bits(8191, 13)  # length 258, distance 24577 + 8191 = 32768
    fixed_lit(b, 256)
    inflate_ok(zwrap(b.done(), head + head[:258]), head + head[:258])


def test_inflate_the_stored_whole_file_vectors():
    """The files kept under tests/golden/png_files/ (the encoder's own streams need a GPU: tests/test_gpu_png_decode.py
    decodes every file png.encode writes for these cases)"""
    stored = [c for c in FC.CASES if c.get("stored")]
    assert stored
    for c in stored:
        idat, _ = FC.parse(FC.stored_file(c))
        z = b"".join(idat)
        want = zlib.decompress(z)
        assert decode.inflate_zlib(z, len(want)) == want, c["name"]


def dynamic_header(b, hlit, hdist, cl_lengths):
    """BTYPE 2, counts, and the 19 code-length code lengths (all sent, in the format's order)"""
    b.bits(1, 1).bits(2, 2).bits(hlit - 257, 5).bits(hdist - 1, 5).bits(15, 4)
    for s in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]:
        b.bits(cl_lengths.get(s, 0), 3)
    return b


def crafted_errors():
    e = {}
    e["zlib stream too short"] = b"\x78\x9c\x03\x00\x00"
    e["invalid zlib compression method"] = b"\x77\x9c" + bytes(8)
    e["invalid zlib header checksum"] = b"\x78\x9d" + bytes(8)
    e["reserved block type"] = zwrap(b"\x07")
    e["stored block LEN/NLEN mismatch"] = zwrap(b"\x01\x05\x00\x00\x00hello")
    e["unexpected end of stream"] = zwrap(b"\x01\x05\x00\xfa\xffhel")
    # fixed block: length code then distance symbol 30
    b = BitsOut().bits(1, 1).bits(1, 2)
    fixed_lit(b, 65)
    fixed_lit(b, 257).code(30, 5)
    e["invalid distance code"] = zwrap(b.done() + bytes(4))
    b = BitsOut().bits(1, 1).bits(1, 2)
    fixed_lit(b, 65)
    fixed_lit(b, 257).code(1, 5)  # distance 2 with one byte out
    e["distance too far back"] = zwrap(b.done() + bytes(4))
    b = BitsOut().bits(1, 1).bits(1, 2)
    fixed_lit(b, 286)
    e["invalid literal/length code: 286"] = zwrap(b.done() + bytes(4))
    # dynamic: code-length code {16: 1 bit, 0: 1 bit}; the first symbol is a repeat
    b = dynamic_header(BitsOut(), 257, 1, {0: 1, 16: 1})
    b.code(1, 1)  # (canonical: symbol 0 -> 0, symbol 16 -> 1)
    e["repeat code at start"] = zwrap(b.done() + bytes(4))
    # ... {0: 1 bit, 18: 1 bit}: 258 lengths wanted, 2 x 138 zeros sent
    b = dynamic_header(BitsOut(), 257, 1, {0: 1, 18: 1})
    b.code(1, 1).bits(127, 7).code(1, 1).bits(127, 7)
    e["too many code lengths"] = zwrap(b.done() + bytes(4))
    # ... all 258 lengths zero: the literal table is empty
    b = dynamic_header(BitsOut(), 257, 1, {0: 1, 18: 1})
    b.code(1, 1).bits(127, 7).code(1, 1).bits(120 - 11, 7)
    e["empty Huffman table"] = zwrap(b.done() + bytes(4))
    # ... one literal code of one bit (symbol 0 -> "0"): the bit 1 is no code
    b = dynamic_header(BitsOut(), 257, 1, {0: 1, 1: 2, 18: 2})  # canonical: 0 -> 0, 1 -> 10, 18 -> 11
    b.code(2, 2).code(3, 2).bits(127, 7).code(3, 2).bits(119 - 11, 7)  # length 1 for symbol 0, then 257 zeros
    b.code(1, 1)
    e["invalid Huffman code"] = zwrap(b.done() + bytes(4))
    return e


ERRORS = crafted_errors()


@pytest.mark.parametrize("message", sorted(ERRORS))
def test_every_reachable_inflate_error(message):
    with pytest.raises(error.InvalidDecode) as e:
        decode.inflate_zlib(ERRORS[message], 4)
    assert str(e.value) == "Decode error: " + message


def test_preset_dictionary_is_unsupported():
    with pytest.raises(error.UnsupportedDecode) as e:
        decode.inflate_zlib(b"\x78\xbb" + bytes(8), 4)
    assert str(e.value) == "Unsupported: preset dictionary not supported"


def test_adler_is_read_from_the_last_four_bytes_and_comes_before_the_size():
    data = lcg(1000, 6)
    z = zlib.compress(data, 6)
    bad = z[:-1] + bytes([z[-1] ^ 0x5A])
    with pytest.raises(error.InvalidDecode) as e:
        decode.inflate_zlib(bad, len(data))
    stored = struct.unpack(">I", bad[-4:])[0]
    assert str(e.value) == "Decode error: Adler32 mismatch: expected %08X, got %08X" % (stored, zlib.adler32(data))
    # bytes between the final block and the checksum are not read: the last four bytes are the checksum
    inflate_ok(z[:-4] + b"junk" + z[-4:], data)
    # a wrong size AND a wrong checksum: the checksum is reported
    with pytest.raises(error.InvalidDecode) as e:
        decode.inflate_zlib(bad, len(data) + 1)
    assert "Adler32 mismatch" in str(e.value)
    for png, expected in [(bad, len(data)), (z, len(data) - 1), (z, len(data) + 1)]:
        try:
            M.inflate_zlib(png, expected)
            raise AssertionError("the model accepted it")
        except M.DecodeError as want:
            with pytest.raises(error.InvalidDecode) as e:
                decode.inflate_zlib(png, expected)
            assert str(e.value) == str(want)


def test_a_stream_longer_than_expected_never_writes_past_it():
    """One byte long, and much longer with matches that reach back across the end of the buffer: size mismatch with the
    stream's true length, the bytes behind the buffer untouched"""
    from pixo_amd import _lib
    L = _lib.load()
    for data, expected in [(lcg(500, 7), 499), ((lcg(300, 8) * 400), 1000), (bytes(100000), 5)]:
        z = zlib.compress(data, 9)
        out = np.full(expected + 64, 0xA5, np.uint8)
        f = np.frombuffer(z, np.uint8)
        rc = L.pixo_hip_zlib_inflate(f.ctypes.data, f.size, out.ctypes.data, expected)
        assert rc == M.INVALID_DECODE
        assert L.pixo_hip_last_error().decode() == "Decode error: decompressed size mismatch: expected %d, got %d" % (expected, len(data))
        assert out[:expected].tobytes() == data[:expected] and (out[expected:] == 0xA5).all()
