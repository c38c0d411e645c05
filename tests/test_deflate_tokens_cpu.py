"""The tools of the DEFLATE audit proved without a GPU: the reader (tests/deflate_tokens.py) against zlib's own streams in
every strategy and against hand-corrupted ones; the model of today's finder through the host build of the block
assembler and back through the reader; the condition each case of tests/deflate_cases.py is named after; the audit's layers
on the model's own stream; the length limiter against package-merge."""
import struct
import zlib

import pytest

import deflate_audit as A
import deflate_cases as C
import deflate_reference as R
import deflate_tokens as T
import emu_png_deflate_lib as E
import test_emu_png_deflate as TE

STRATEGIES = [("level0", 0, zlib.Z_DEFAULT_STRATEGY), ("level1", 1, zlib.Z_DEFAULT_STRATEGY), ("level6", 6, zlib.Z_DEFAULT_STRATEGY),
              ("level9", 9, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("rle", 6, zlib.Z_RLE), ("huffman_only", 6, zlib.Z_HUFFMAN_ONLY)]


def zlib_streams(data):
    for name, level, strategy in STRATEGIES:
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
        yield name, c.compress(data) + c.flush()
    c = zlib.compressobj(6)
    half = len(data) // 2
    yield "full_flush", c.compress(data[:half]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[half:]) + c.flush()


def check_read(stream, data):
    z = T.read_zlib(stream)
    assert z.data == data and b"".join(b.data for b in z.blocks) == data
    assert (z.end + 7) // 8 == len(stream) - 4 and z.adler32 == zlib.adler32(data)
    for b in z.blocks:
        assert b.start < b.first_token <= b.end
        if b.btype != T.STORED:
            assert T.token_bytes(b.tokens, data[:b.out_start]) == b.data
            at = b.first_token
            for off, w in zip(b.offsets, b.widths):  # the tokens tile the body
                assert off == at
                at += w
            assert at == b.eob_offset and b.eob_offset + b.eob_width == b.end
    return z


@pytest.mark.parametrize("name", C.NAMES)
def test_reader_against_zlib(name):
    _, data, _, _ = C.get(name)
    for strategy, stream in zlib_streams(data):
        z = check_read(stream, data)
        forms = {b.btype for b in z.blocks}
        if strategy == "level0":
            assert forms == {T.STORED}
        if strategy == "fixed":
            assert T.DYNAMIC not in forms  # (zlib still stores what the fixed code would enlarge)
        if strategy == "full_flush":  # the empty stored block the kernel puts behind a block: 000, padding, 00 00 FF FF
            empty = [b for b in z.blocks if b.btype == T.STORED and b.data == b""]
            assert len(empty) == 1 and not empty[0].final and empty[0].end % 8 == 0 and stream[empty[0].end // 8 - 4:empty[0].end // 8] == b"\x00\x00\xff\xff"


def test_reader_meets_every_form():
    _, data, _, _ = C.get("wide_tokens")
    forms = set()
    for _, stream in zlib_streams(data):
        forms |= {b.btype for b in T.read_zlib(stream).blocks}
    assert forms == {T.STORED, T.FIXED, T.DYNAMIC}


def wrap(bits):
    """A string of '0' / '1' in stream order -> a zlib stream around these DEFLATE bits (the checksum is not looked at)."""
    bits += "0" * (-len(bits) % 8)
    return b"\x78\x9c" + bytes(int(bits[i:i + 8][::-1], 2) for i in range(0, len(bits), 8)) + b"\0\0\0\1"


def lsb(value, n):
    return format(value, "0%db" % n)[::-1] if n else ""


def test_corrupted_streams_raise():
    good = zlib.compress(b"stored bytes", 0)
    assert T.read_zlib(good).data == b"stored bytes"
    flipped = bytearray(good)
    flipped[5] ^= 0x10  # NLEN
    with pytest.raises(T.FormatError, match="NLEN"):
        T.read_zlib(bytes(flipped))
    with pytest.raises(T.FormatError, match="padding"):
        T.read_zlib(wrap("1" + "00" + "10000" + lsb(0, 16) + lsb(0xFFFF, 16)))
    head = "1" + "01"  # a final dynamic block: HLIT 257, HDIST 1, HCLEN 4 — code-length lengths for 16, 17, 18, 0
    with pytest.raises(T.FormatError, match="over-subscribed"):
        T.read_zlib(wrap(head + lsb(0, 5) + lsb(0, 5) + lsb(0, 4) + lsb(1, 3) + lsb(1, 3) + lsb(1, 3) + lsb(0, 3)))  # Kraft sum 3/2
    with pytest.raises(T.FormatError, match="incomplete"):
        T.read_zlib(wrap(head + lsb(0, 5) + lsb(0, 5) + lsb(0, 4) + lsb(2, 3) + lsb(2, 3) + lsb(0, 3) + lsb(0, 3)))
    fixed = "1" + "10"  # a final fixed block; Huffman codes go in most significant bit first
    with pytest.raises(T.FormatError, match="before the start"):
        T.read_zlib(wrap(fixed + "0000001" + "00000"))  # length 3 at distance 1 as the first token
    with pytest.raises(T.FormatError, match="before the start"):
        T.read_zlib(wrap(fixed + "00110000" + "0000001" + "00001"))  # one literal, then distance 2
    assert T.read_zlib(wrap(fixed + "00110000" + "0000001" + "00000" + "0000000")).data == b"\0\0\0\0"
    with pytest.raises(T.FormatError, match="symbol 286"):
        T.read_zlib(wrap(fixed + "11000110"))
    with pytest.raises(T.FormatError, match="distance symbol 30"):
        T.read_zlib(wrap(fixed + "00110000" + "0000001" + "11110"))
    with pytest.raises(T.FormatError, match="ends inside"):
        T.read_zlib(wrap(fixed + "00110000"))
    with pytest.raises(T.FormatError, match="block type 3"):
        T.read_zlib(wrap("111"))


# ---- the model of today's finder through the block assembler and back ------------------------------------------------------

_ASSEMBLED = {}


def assembled(name):
    """-> (zlib stream of the model's tokens: one block per chunk in the smallest form as the host build of the kernel's
    step 3 chooses it, the forms chosen)"""
    if name not in _ASSEMBLED:
        _, data, bpp, row = C.get(name)
        tokens, _ = C.model(name)
        out, forms = bytearray(E.zlib_header(6)), []
        for k, chunk_tokens in enumerate(tokens):
            chunk = data[k * R.CHUNK:(k + 1) * R.CHUNK]
            blk, chosen = E.block(A.emu_tokens(chunk_tokens), chunk, E.SMALLEST, k == len(tokens) - 1)
            out += blk
            forms.append(chosen)
        _ASSEMBLED[name] = (bytes(out) + struct.pack(">I", zlib.adler32(data)), forms)
    return _ASSEMBLED[name]


@pytest.mark.parametrize("name", C.NAMES)
def test_model_through_the_block_assembler(name):
    _, data, bpp, row = C.get(name)
    tokens, offered = C.model(name)
    stream, forms = assembled(name)
    assert zlib.decompress(stream) == data
    for chunk_tokens in tokens:
        assert T.token_bytes(chunk_tokens, data[:chunk_tokens[0][0]]) == data[chunk_tokens[0][0]:chunk_tokens[0][0] + R.CHUNK]
    z = check_read(stream, data)
    cs = A.chunks_of(z, data)
    assert [b.btype for b, _, _, _ in cs] == forms
    for (b, c0, n, last), chunk_tokens in zip(cs, tokens):
        assert b.data == data[c0:c0 + n]
        if b.btype != T.STORED:
            assert b.tokens == chunk_tokens
    A.all_layers(stream, data, bpp, row, tokens, offered)  # the audit's layers hold on the model's own stream


def read_assembled(name):
    stream, _ = assembled(name)
    _, data, _, _ = C.get(name)
    z = T.read_zlib(stream)
    return z, A.chunks_of(z, data), data


# ---- every case reaches the edge it is named after -------------------------------------------------------------------------

def test_wide_tokens_reach_the_third_word():
    z, cs, _ = read_assembled("wide_tokens")
    b = cs[0][0]
    assert b.btype == T.DYNAMIC
    late = [(off - b.start, w) for off, w in zip(b.offsets, b.widths) if w + (off - b.start) % 32 > 64]
    assert late, "no token of 34 or more bits that starts late enough in a word; widest %d" % max(b.widths)


def depths(name, which):
    _, cs, _ = read_assembled(name)
    return [R.huffman_cost(R.histograms(b.tokens)[which])[1] for b, _, _, _ in cs if b.btype != T.STORED]


def test_deep_cases_need_the_limiter():
    assert max(depths("deep_literals", 0)) > 15
    assert max(depths("deep_distances", 1)) > 15
    _, cs, _ = read_assembled("deep_distances")
    assert cs[0][0].btype == T.DYNAMIC and max(cs[0][0].dist_lens) == 15 and max(cs[0][0].lit_lens) < 15
    _, cs, _ = read_assembled("deep_literals")
    assert cs[1][0].btype == T.DYNAMIC and max(cs[1][0].lit_lens) == 15 and not [t for t in cs[1][0].tokens if len(t) == 2]
    assert max(depths("fibonacci_literals", 0)) == 13  # the input that was thought to reach the limiter does not


@pytest.mark.parametrize("name", [n for n in C.NAMES if n.startswith(("chunk_", "window_"))])
def test_matches_reach_into_the_chunk_before(name):
    _, cs, _ = read_assembled(name)
    reach = [t for b, c0, _, _ in cs[1:] for t in b.tokens if len(t) == 3 and t[0] - t[2] < c0 and (t[1] > 4 or name.startswith("chunk_"))]  # (4 in noise: an accidental repeat)
    if name in ("chunk_65534", "chunk_65535", "chunk_65536", "chunk_65538", "window_32769_straddle", "window_32769_early"):
        assert not reach  # one chunk; a second chunk of 1 or 3 bytes, too short to hash; a marker one byte out of reach
    else:
        assert reach
    if name.startswith("chunk_"):
        b, c0, n, _ = cs[0]
        assert b.tokens[-1][0] + b.tokens[-1][1] == n and 3 <= b.tokens[-1][1] < 258, "no match cut by the end of the first chunk"


@pytest.mark.parametrize("dist", [32767, 32768, 32769])
@pytest.mark.parametrize("where", ["early", "straddle"])
def test_window_marker(dist, where):
    name = "window_%d_%s" % (dist, where)
    first, second, total = C.window_layout(dist, where)
    _, data, _, _ = C.get(name)
    assert len(data) == total and data[first:first + C.WINDOW_MARKER] == data[second:second + C.WINDOW_MARKER]
    _, cs, _ = read_assembled(name)
    assert all(b.btype == T.DYNAMIC for b, _, _, _ in cs)  # the tokens can be read
    inside = [t for b, _, _, _ in cs for t in b.tokens if second <= t[0] < second + C.WINDOW_MARKER]
    c1 = cs[1][1]
    if dist == 32769:  # one byte out of reach: literals (an accidental repeat of the noise apart)
        assert not [t for t in inside if len(t) == 3 and t[2] >= 32768] and len([t for t in inside if len(t) == 2]) > C.WINDOW_MARKER - 10
    elif where == "early":  # window start above zero; the whole marker through the seeded table
        assert inside == [(second, 258, dist), (second + 258, C.WINDOW_MARKER - 258, dist)]
    else:  # cut by the chunk's end, found again at the first position of the next chunk: the first seeded position at 32768
        assert inside == [(second, c1 - second, dist), (c1, C.WINDOW_MARKER - (c1 - second), dist)]


def test_substeps_see_only_earlier_substeps():
    for n in (1023, 1024, 1025, 1027, 1028):
        _, cs, _ = read_assembled("substep_%d" % n)
        tokens = C.model("substep_%d" % n)[0][0]
        assert all(len(t) == 2 for t in tokens if t[0] < 1024), "a match before the table has any entry"
        tail = [t for t in tokens if t[0] >= 1024]
        if n == 1028:  # the first position that has four bytes to hash and an earlier sub-step to find them in
            assert tail == [(1024, 4, 300)]
        else:
            assert len(tail) == n - min(n, 1024) and all(len(t) == 2 for t in tail)


def test_segment_straddle_enters_segments_midway():
    _, cs, _ = read_assembled("segment_straddle")
    tokens = cs[0][0].tokens
    assert any(len(t) == 3 and (t[0] + t[1]) // 64 >= t[0] // 64 + 2 for t in tokens), "no token that skips a whole segment"
    starts = {t[0] for t in tokens}
    for p, length, dist in C.segment_straddle_plan():
        assert (p, length, dist) in tokens, "the planted match at %d (%d mod 64) is not in the parse" % (p, p % 64)
        assert p + length in starts


def test_len3_rule_at_4096():
    kept = [t for t in C.model("len3_row4096")[0][0] if len(t) == 3]
    assert [t for t in kept if t[2] == 4096] == [(p, 3, 4096) for p in C.LEN3_POSITIONS]
    assert not [t for t in C.model("len3_row4097")[0][0] if len(t) == 3 and t[1] == 3]  # (one accidental 4-byte repeat of the noise apart)
    _, data, _, row = C.get("len3_row4097")
    assert all(R.longest(data, p, row, 258) == 3 for p in C.LEN3_POSITIONS)


def test_tie_goes_to_the_smaller_distance():
    _, data, bpp, row = C.get("tie_period7")
    tokens = C.model("tie_period7")[0][0]
    assert R.longest(data, 100, bpp, 258) == R.longest(data, 100, row, 258) == 211 - 100  # a tie below the cap
    assert R.explicit_best(data, 0, len(data), 100, bpp, row) == (111, 14)
    matches = [t for t in tokens if len(t) == 3]
    assert any(t[2] == 14 and t[1] < 258 for t in matches)  # (21 is right where 14 runs into the break first)


def test_form_ties():
    for name, sizes, want in (("form_tie_fixed_dynamic", (35, 32, 32), T.FIXED), ("form_tie_all", (90, 90, 90), T.STORED)):
        _, data, _, _ = C.get(name)
        tokens = C.model(name)[0][0]
        dynamic = len(E.block(A.emu_tokens(tokens), data, E.DYNAMIC, True)[0])
        assert (R.stored_cost(len(data)), R.form_bytes(R.fixed_cost(tokens), True), dynamic) == sizes
        assert assembled(name)[1] == [want]


def test_tiny_inputs():
    for k in range(1, 10):
        tokens = C.model("tiny_%d" % k)[0][0]
        assert tokens == [(i, (i % 3) * 50 + 1) for i in range(min(k, 3))] + ([(3, k - 3, 3)] if k >= 6 else [(i, (i % 3) * 50 + 1) for i in range(3, k)])


def test_every_form_is_chosen_by_some_case():
    chosen = {}
    for name in C.NAMES:
        for f in assembled(name)[1]:
            chosen.setdefault(f, name)
    assert set(chosen) == {E.STORED, E.FIXED, E.DYNAMIC}, chosen


# ---- the limiter against package-merge -------------------------------------------------------------------------------------

def histograms_of_all_cases():
    for name in C.NAMES:
        for k, tokens in enumerate(C.model(name)[0]):
            lit, dist, _ = R.histograms(tokens)
            yield "%s/%d/lit" % (name, k), lit, 15
            yield "%s/%d/dist" % (name, k), dist, 15
    for name, freq in sorted(TE.ALPHABETS.items()):
        yield "alphabet/%s" % name, freq, 15
        yield "alphabet/%s/19" % name, (TE.fibonacci(19) if name == "fibonacci30" else freq[:19]), 7


# Bits by which the limiter's code is dearer than the optimal length-limited code, per histogram where it is dearer at all.
# Measured from package_merge_cost; integer arithmetic, so the margin is zero.  Whoever changes the limiter records it again.
LIMITER_EXCESS = {
    "alphabet/fibonacci30": 9354,
    "alphabet/fibonacci30/19": 3194,
}


def test_limiter_against_package_merge():
    excess = {}
    for key, freq, limit in histograms_of_all_cases():
        lens = [int(v) for v in E.huffman_lengths(freq, limit)]
        used = sum(1 for f in freq if f)
        cost = sum(f * l for f, l in zip(freq, lens))
        assert max(lens) <= limit
        assert E.kraft(lens) == 1 << 15, key  # (emu scales by 2^15 whatever the limit)
        best, depth = R.huffman_cost(freq)
        pm = R.package_merge_cost(freq, limit)
        assert pm >= best and cost >= pm, key
        if used >= 2:
            assert all(bool(f) == bool(l) for f, l in zip(freq, lens)), key
        if depth <= limit:
            assert pm == best and cost == best, "%s: %d bits where an optimal code of depth %d costs %d" % (key, cost, depth, best)
        if cost > pm:
            excess[key] = cost - pm
    assert excess == LIMITER_EXCESS
