"""zlib streams for the device inflate's tests (pixo_amd/csrc/png_inflate.hip, png_inflate_math.h), each named for the boundary
it sits on: a stream, the size the caller expects, and what the bytes are — from `zlib` where zlib wrote the stream, from a
token-by-token model here where the stream is written by hand with this file's own bit writer.  `cases(step_tokens,
window_bytes, far_distance, stored_chunk)` places them by the kernel's exported constants.  Test harness only.

A case: dict(name, z, expected, data, kind).  kind "ok": the stream inflates to `data` (len(data) == expected); "bad": no
inflate accepts it at that size (data None); "needs_host": a code set is over-subscribed — the device leaves it to the host,
whose bytes are `data`; "header": the zlib header itself is refused (the batch driver never sends such a stream to the device)."""
import struct
import zlib

import synth


# ---- bits ----------------------------------------------------------------------------------------------------------------------
class Bits:
    """DEFLATE's bit order: fields go in from the least significant bit, Huffman codes from their most significant bit"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, count):
        for i in range(count):
            self.acc |= ((value >> i) & 1) << self.n
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                self.acc, self.n = 0, 0
        return self

    def code(self, value, count):
        for i in reversed(range(count)):
            self.bits((value >> i) & 1, 1)
        return self

    def align(self):
        if self.n:
            self.out.append(self.acc)
            self.acc, self.n = 0, 0
        return self

    def raw(self, data):
        assert self.n == 0
        self.out += data
        return self

    def done(self):
        return bytes(self.align().out)


LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def length_symbol(length):
    s = max(i for i in range(29) if LENGTH_BASE[i] <= length) if length < 258 else 28
    return 257 + s, LENGTH_EXTRA[s], length - LENGTH_BASE[s]


def distance_symbol(distance):
    s = max(i for i in range(30) if DIST_BASE[i] <= distance)
    return s, DIST_EXTRA[s], distance - DIST_BASE[s]


def canonical(lengths):
    """{symbol: length} -> {symbol: (code, length)} (RFC 1951 3.2.2); lengths of 0 have no code"""
    codes, code = {}, 0
    for n in range(1, 16):
        for s in sorted(lengths):
            if lengths[s] == n:
                codes[s] = (code, n)
                code += 1
        code <<= 1
    return codes


FIXED_LIT = canonical({s: (8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8) for s in range(288)})
FIXED_DIST = canonical({s: 5 for s in range(32)})


def put_tokens(b, tokens, lit, dist):
    """tokens: ints (literals) and (length, distance) pairs, then the end-of-block code"""
    for t in tokens:
        if isinstance(t, int):
            b.code(*lit[t])
        else:
            s, eb, ev = length_symbol(t[0])
            b.code(*lit[s]).bits(ev, eb)
            s, eb, ev = distance_symbol(t[1])
            b.code(*dist[s]).bits(ev, eb)
    return b.code(*lit[256])


def fixed_block(b, tokens, final=True):
    return put_tokens(b.bits(1 if final else 0, 1).bits(1, 2), tokens, FIXED_LIT, FIXED_DIST)


def dynamic_block(b, lit_lengths, dist_lengths, tokens, final=True, hlit=None, hdist=None):
    """A dynamic block whose code-length code gives the symbols 0..15 four bits each (a complete set; no repeat codes): every
    length is sent as it is"""
    hlit = max(257, max(lit_lengths) + 1) if hlit is None else hlit
    hdist = max(1, max(dist_lengths) + 1 if dist_lengths else 1) if hdist is None else hdist
    b.bits(1 if final else 0, 1).bits(2, 2).bits(hlit - 257, 5).bits(hdist - 1, 5).bits(19 - 4, 4)
    for s in CL_ORDER:
        b.bits(4 if s < 16 else 0, 3)
    cl = canonical({s: 4 for s in range(16)})
    for s in range(hlit):
        b.code(*cl[lit_lengths.get(s, 0)])
    for s in range(hdist):
        b.code(*cl[dist_lengths.get(s, 0)])
    return b


def run_tokens(tokens, before=b""):
    """What the tokens produce behind `before`"""
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, distance = t
            assert 3 <= length <= 258 and 1 <= distance <= len(out)
            for _ in range(length):
                out.append(out[-distance])
    return bytes(out[len(before):])


def zwrap(body, data=b"", adler=None):
    return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(data) if adler is None else adler)


def stored(data, final=True):
    return bytes([1 if final else 0]) + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data


def lcg(n, seed):
    return synth.lcg_bytes(n, seed).tobytes()


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush=zlib.Z_FINISH):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush(flush)


def text(n, seed):
    """Compressible bytes: words drawn from a small vocabulary"""
    words = [lcg(3 + k % 7, 900 + k) for k in range(40)]
    picks = lcg(n, seed)
    out = bytearray()
    for p in picks:
        out += words[p % 40]
        if len(out) >= n:
            break
    return bytes(out[:n])


# ---- the error streams of tests/test_png_decode_cpu.py crafted_errors(), restated ------------------------------------------------
def _cl_header(b, hlit, hdist, cl_lengths):
    b.bits(1, 1).bits(2, 2).bits(hlit - 257, 5).bits(hdist - 1, 5).bits(15, 4)
    for s in CL_ORDER:
        b.bits(cl_lengths.get(s, 0), 3)
    return b


def error_streams():
    """message of the host inflate -> stream (every one asked for 4 bytes)"""
    e = {}
    e["zlib stream too short"] = b"\x78\x9c\x03\x00\x00"
    e["invalid zlib compression method"] = b"\x77\x9c" + bytes(8)
    e["invalid zlib header checksum"] = b"\x78\x9d" + bytes(8)
    e["reserved block type"] = zwrap(b"\x07")
    e["stored block LEN/NLEN mismatch"] = zwrap(b"\x01\x05\x00\x00\x00hello")
    e["unexpected end of stream"] = zwrap(b"\x01\x05\x00\xfa\xffhel")
    b = Bits().bits(1, 1).bits(1, 2).code(*FIXED_LIT[65]).code(*FIXED_LIT[257]).code(30, 5)
    e["invalid distance code"] = zwrap(b.done() + bytes(4))
    b = Bits().bits(1, 1).bits(1, 2).code(*FIXED_LIT[65]).code(*FIXED_LIT[257]).code(1, 5)  # distance 2 with one byte out
    e["distance too far back"] = zwrap(b.done() + bytes(4))
    b = Bits().bits(1, 1).bits(1, 2).code(*FIXED_LIT[286])
    e["invalid literal/length code: 286"] = zwrap(b.done() + bytes(4))
    b = _cl_header(Bits(), 257, 1, {0: 1, 16: 1}).code(1, 1)  # the first symbol is a repeat
    e["repeat code at start"] = zwrap(b.done() + bytes(4))
    b = _cl_header(Bits(), 257, 1, {0: 1, 18: 1}).code(1, 1).bits(127, 7).code(1, 1).bits(127, 7)  # 2 x 138 zeros for 258 lengths
    e["too many code lengths"] = zwrap(b.done() + bytes(4))
    b = _cl_header(Bits(), 257, 1, {0: 1, 18: 1}).code(1, 1).bits(127, 7).code(1, 1).bits(120 - 11, 7)  # all 258 lengths zero
    e["empty Huffman table"] = zwrap(b.done() + bytes(4))
    b = _cl_header(Bits(), 257, 1, {0: 1, 1: 2, 18: 2})  # canonical: 0 -> 0, 1 -> 10, 18 -> 11
    b.code(2, 2).code(3, 2).bits(127, 7).code(3, 2).bits(119 - 11, 7).code(1, 1)  # symbol 0 has the one code "0": the bit 1 is none
    e["invalid Huffman code"] = zwrap(b.done() + bytes(4))
    return e


HEADER_ERRORS = ("zlib stream too short", "invalid zlib compression method", "invalid zlib header checksum")


def oversubscribed_stream(count=4):
    """Three literal/length symbols of one bit each: 1, 2 and 256.  The host fills its lookup in symbol order — 1 gets code 0, 2
    gets code 1, 256 gets code 2, whose one reversed bit is 0 again and overwrites symbol 1 — so the bit 1 is symbol 2 and the
    bit 0 ends the block: `count` ones and a zero inflate to `count` bytes of value 2.  -> (stream, data)"""
    b = dynamic_block(Bits(), {1: 1, 2: 1, 256: 1}, {}, [])
    for _ in range(count):
        b.bits(1, 1)
    b.bits(0, 1)
    data = bytes([2]) * count
    return zwrap(b.done(), data), data


def case(name, z, data, kind="ok", expected=None):
    return dict(name=name, z=z, expected=len(data) if expected is None else expected, data=data, kind=kind, zlib_refuses=False)


def cases(step_tokens=64, window_bytes=32768, far_distance=16256, stored_chunk=4096):
    W = window_bytes
    out = []
    # tiny streams
    out.append(case("tiny_empty", zlib.compress(b"", 6), b""))
    out.append(case("tiny_one_byte", zlib.compress(b"a", 6), b"a"))
    # stored blocks
    out.append(case("stored_0_bytes", zwrap(stored(b"")), b""))
    big = lcg(65535, 11)
    out.append(case("stored_65535_bytes", zwrap(stored(big), big), big))
    for n in (stored_chunk - 1, stored_chunk, stored_chunk + 1):
        d = lcg(n, 12)
        out.append(case("stored_%d_bytes_at_the_copy_chunk" % n, zwrap(stored(d), d), d))
    tail = lcg(300, 13)
    b = fixed_block(Bits(), [65], final=False)  # 3 + 8 + 7 bits: the block ends mid-byte
    assert b.n != 0
    z = b.bits(1, 1).bits(0, 2).align().raw(stored(tail)[1:]).done()  # the stored header's three bits share the byte, then the padding
    out.append(case("stored_behind_a_huffman_block_that_ended_mid_byte", zwrap(z, b"A" + tail), b"A" + tail))
    t = text(9000, 14)
    z = stored(t[:100], False) + raw_deflate(t[100:4000], 6, zlib.Z_FIXED, zlib.Z_FULL_FLUSH) + raw_deflate(t[4000:], 9)
    out.append(case("stored_fixed_dynamic_in_one_stream", zwrap(z, t), t))
    both = text(40000, 15) + lcg(5000, 16)
    c = zlib.compressobj(6)
    z = c.compress(both[:20000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(both[20000:]) + c.flush()
    out.append(case("z_full_flush", z, both))
    # match extremes
    tok = [65, (258, 1)]
    out.append(case("match_258_at_distance_1", zwrap(fixed_block(Bits(), tok).done(), run_tokens(tok)), run_tokens(tok)))
    head = lcg(W, 17)
    tok = list(head) + [(258, W)]
    out.append(case("distance_%d_at_offset_%d" % (W, W), zwrap(fixed_block(Bits(), tok).done(), run_tokens(tok)), run_tokens(tok)))
    b = Bits().bits(1, 1).bits(1, 2).code(*FIXED_LIT[65]).code(*FIXED_LIT[257]).code(1, 5).code(*FIXED_LIT[256])
    out.append(case("distance_one_past_the_output", zwrap(b.done() + bytes(4)), None, "bad", expected=4))
    tok = list(lcg(13, 18)) + [(7, 13), (30, 5), 9, (40, 33), (3, 1)]  # matches that begin, end and lie across multiples of 16
    out.append(case("matches_across_16_byte_pieces", zwrap(fixed_block(Bits(), tok).done(), run_tokens(tok)), run_tokens(tok)))
    # step boundaries
    for n in (step_tokens - 1, step_tokens, step_tokens + 1, 2 * step_tokens + 1):
        tok = list(lcg(n, 19))
        out.append(case("literal_tokens_%d" % n, zwrap(fixed_block(Bits(), tok).done(), bytes(tok)), bytes(tok)))
        tok = list(lcg(n - 2, 20)) + [(5, 3), (200, n - 1)]  # ... the last token(s) on either side of the step are matches
        out.append(case("tokens_%d_ending_in_matches" % n, zwrap(fixed_block(Bits(), tok).done(), run_tokens(tok)), run_tokens(tok)))
    tok = [1, 2, 3, (3, 3), (4, 2), (258, 7), 9, (17, 1), (64, 64), (65, 64), (130, 63), (100, 300)]
    out.append(case("sources_are_literals_and_matches_of_the_same_step", zwrap(fixed_block(Bits(), tok).done(), run_tokens(tok)), run_tokens(tok)))
    # a literal directly behind a match that reaches almost a window back: its ring slot is one of the match's source bytes
    far = []
    for dist in (W - 3, far_distance, far_distance + 1, W):
        far += [(10, dist), 200, 201, 202, (258, dist), 7]
    tok = list(lcg(W, 21)) + far
    out.append(case("literals_behind_far_matches", zwrap(fixed_block(Bits(), tok).done(), run_tokens(tok)), run_tokens(tok)))
    # ring boundaries: matches across the wrap
    for n in (W - 1, W, W + 1, 2 * W + 1):
        d = text(n, 22 + n % 7)
        out.append(case("window_output_%d" % n, zlib.compress(d, 9), d))
    d = lcg(300, 30) * ((2 * W + 700) // 300)
    out.append(case("window_long_period_matches", zlib.compress(d, 6), d))
    # code sets
    lit15 = {s: s + 1 for s in range(12)}  # 1/2 + ... + 2^-12, then 2^-13 + 2^-14 + 2 * 2^-15: complete, two codes of 15 bits
    lit15.update({12: 13, 256: 14, 257: 15, 269: 15})  # (257: length 3, 269: lengths 19..22)
    tok = [0, 1, 12, 11, 12, 2, (3, 2), 12, 10, (20, 5), 0, (22, 2)]
    b = dynamic_block(Bits(), lit15, {1: 1, 4: 1}, [])
    z = put_tokens(b, tok, canonical(lit15), canonical({1: 1, 4: 1})).done()
    out.append(case("dynamic_15_bit_codes", zwrap(z, run_tokens(tok)), run_tokens(tok)))
    lit = {s: 3 for s in range(6)}
    lit.update({256: 3, 257: 3})  # complete; length symbol 257 is length 3
    tok = [0, 1, 2, (3, 3), 5, (3, 3)]
    b = dynamic_block(Bits(), lit, {2: 1}, [])  # distance symbol 2 (distance 3) has the only distance code, of one bit: incomplete
    z = put_tokens(b, tok, canonical(lit), canonical({2: 1})).done()
    out.append(case("single_distance_code_of_one_bit", zwrap(z, run_tokens(tok)), run_tokens(tok)))
    z, d = oversubscribed_stream()
    out.append(case("oversubscribed_literal_set", z, d, "needs_host"))
    # zlib's strategies and levels on filtered-image-like bytes
    img = bytes((3 * (i % 97) + (i // 289)) & 255 for i in range(50000)) + lcg(3000, 31)
    for name, level, strategy in (("z_fixed", 6, zlib.Z_FIXED), ("z_huffman_only", 6, zlib.Z_HUFFMAN_ONLY), ("z_rle", 6, zlib.Z_RLE),
                                  ("z_level_1", 1, zlib.Z_DEFAULT_STRATEGY), ("z_level_9", 9, zlib.Z_DEFAULT_STRATEGY)):
        out.append(case(name, zwrap(raw_deflate(img, level, strategy), img), img))
    # stream tail, wrong sizes
    z = zlib.compress(t, 6)
    out.append(case("junk_between_final_block_and_checksum", z[:-4] + b"junk" + z[-4:], t))  # (zlib itself wants the checksum at once)
    out[-1]["zlib_refuses"] = True
    out.append(case("expected_one_short", z, None, "bad", expected=len(t) - 1))
    out.append(case("expected_one_long", z, None, "bad", expected=len(t) + 1))
    # the host inflate's error streams
    for message, z in sorted(error_streams().items()):
        out.append(case("error_" + message.replace(" ", "_").replace("/", "_").replace(":", ""), z, None,
                        "header" if message in HEADER_ERRORS else "bad", expected=4))
    out.append(case("error_preset_dictionary", b"\x78\xbb" + bytes(8), None, "header", expected=4))
    assert len({c["name"] for c in out}) == len(out)
    return out
