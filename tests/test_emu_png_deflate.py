"""The host build of pixo_amd/csrc/png_deflate_math.h on its own (no GPU): the length limiter, the code-length code, a
DEFLATE block assembled from a hand-made token list in each of its three forms, the CRC-32 combine."""
import zlib

import numpy as np
import pytest

import emu_png_deflate_lib as E


def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def padded(counts, n):
    return list(counts) + [0] * (n - len(counts))


ALPHABETS = {
    "fibonacci30": padded(fibonacci(30), 286),  # an unlimited Huffman code is 29 deep
    "one": padded([0, 0, 0, 7], 286),
    "two": padded([0, 5, 0, 0, 0, 9], 286),
    "equal286": [3] * 286,
    "zero": [0] * 286,
}


@pytest.mark.parametrize("name", sorted(ALPHABETS))
def test_limiter_15_bits(name):
    freq = ALPHABETS[name]
    lens = E.huffman_lengths(freq, 15)
    assert lens.max() <= 15
    assert E.kraft(lens) <= 32768
    for f, l in zip(freq, lens):
        if f:
            assert l >= 1
    used = [(f, l) for f, l in zip(freq, lens) if f]
    for (fa, la) in used:  # a rarer symbol never has the shorter code
        for (fb, lb) in used:
            if fa < fb:
                assert la >= lb
    if name == "equal286":
        assert sorted(set(lens)) == [8, 9] and E.kraft(lens) == 32768
    if name == "fibonacci30":
        assert lens.max() == 15 and E.kraft(lens) == 32768


@pytest.mark.parametrize("name", sorted(ALPHABETS))
def test_code_length_code_7_bits(name):
    freq = ALPHABETS[name][:19]
    if name == "fibonacci30":
        freq = fibonacci(19)  # unlimited depth 18
    lens = E.huffman_lengths(freq, 7)
    assert lens.max() <= 7
    assert E.kraft(lens) <= 32768
    for f, l in zip(freq, lens):
        if f:
            assert l >= 1


def test_symbol_mapping_matches_rfc1951():
    base_len = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    extra_len = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    base_dist = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                 8193, 12289, 16385, 24577]
    extra_dist = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]
    for length in range(3, 259):
        s = max(i for i in range(29) if base_len[i] <= length)
        if length == 258:
            s = 28
        assert E.symbols(length, 1)[:3] == (257 + s, extra_len[s], length - base_len[s])
    for dist in list(range(1, 600)) + [1024, 1025, 4096, 4097, 24576, 24577, 32767, 32768]:
        s = max(i for i in range(30) if base_dist[i] <= dist)
        assert E.symbols(3, dist)[3:] == (s, extra_dist[s], dist - base_dist[s])


def inflate_raw(block):
    d = zlib.decompressobj(-15)
    out = d.decompress(block)
    return out, d


TEXT = b"the quick brown fox jumps over the lazy dog, the quick brown fox naps. "


def hand_made():
    """(tokens, the bytes they stand for): literals, short and long matches, distance 1 runs, a far match"""
    data = bytearray()
    tokens = []

    def lit(bs):
        for b in bs:
            tokens.append(b)
            data.append(b)

    def mat(length, dist):
        assert 3 <= length <= 258 and 1 <= dist <= len(data)
        tokens.append(E.match(length, dist))
        for _ in range(length):
            data.append(data[-dist])

    lit(TEXT)
    mat(20, len(TEXT))
    lit(b"\x00\xff")
    mat(258, 1)
    mat(3, 2)
    lit(bytes(range(40)))
    mat(11, 40)
    mat(257, 300)
    mat(130, len(data))
    return tokens, bytes(data)


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("mode", [E.STORED, E.FIXED, E.DYNAMIC, E.SMALLEST])
def test_block_round_trip(mode, last):
    tokens, data = hand_made()
    blk, chosen = E.block(tokens, data, mode, last)
    if mode != E.SMALLEST:
        assert chosen == mode
    out, d = inflate_raw(blk + (b"" if last else b"\x01\x00\x00\xff\xff"))
    assert out == data and d.eof and d.unused_data == b""
    if not last:
        assert blk[-4:] == b"\x00\x00\xff\xff" or chosen == E.STORED


@pytest.mark.parametrize("mode", [E.FIXED, E.DYNAMIC])
@pytest.mark.parametrize("data", [b"a", b"aaaaaaaaaaaa", TEXT, bytes(range(256)) * 3], ids=["one_byte", "one_symbol", "text", "all_bytes"])
def test_literal_only_block_round_trip(mode, data):
    blk, _ = E.block(list(data), data, mode, True)
    out, d = inflate_raw(blk)
    assert out == data and d.eof


def test_one_distance_symbol_block():
    data = b"abcdefgh" * 50
    tokens = list(b"abcdefgh") + [E.match(98, 8)] * 4
    blk, _ = E.block(tokens, data, E.DYNAMIC, True)
    assert inflate_raw(blk)[0] == data


def test_smallest_form_is_chosen():
    rng = np.random.RandomState(5)
    noise = rng.randint(0, 256, 3000).astype(np.uint8).tobytes()
    assert E.block(list(noise), noise, E.SMALLEST, True)[1] == E.STORED
    flat = b"\x07" * 3000
    tok = [7] + [E.match(258, 1)] * 11 + [E.match(161, 1)]
    blk, chosen = E.block(tok, flat, E.SMALLEST, True)
    assert chosen in (E.FIXED, E.DYNAMIC) and len(blk) < 40 and inflate_raw(blk)[0] == flat


def test_crc_combine_over_random_splits():
    rng = np.random.RandomState(11)
    for n in (0, 1, 5, 4096, 4097, 70000):
        data = rng.randint(0, 256, n).astype(np.uint8).tobytes()
        assert E.crc32(data) == zlib.crc32(data)
        for _ in range(4):
            cuts = sorted(int(c) for c in rng.randint(0, n + 1, 3))
            parts = [data[a:b] for a, b in zip([0] + cuts, cuts + [n])]
            crc = zlib.crc32(b"IDAT")
            for p in parts:
                crc = E.crc32_combine(crc, zlib.crc32(p), len(p))
            assert crc == zlib.crc32(b"IDAT" + data)


def test_zlib_header_and_bound():
    # FLEVEL 1 / 2 / 3 for levels <= 2 / <= 6 / above, level clamped to 1..9; FCHECK makes the pair a multiple of 31
    want = {0: b"\x78\x5e", 1: b"\x78\x5e", 2: b"\x78\x5e", 3: b"\x78\x9c", 6: b"\x78\x9c", 7: b"\x78\xda", 9: b"\x78\xda", 200: b"\x78\xda"}
    for level, h in want.items():
        assert E.zlib_header(level) == h and (h[0] * 256 + h[1]) % 31 == 0
    for n in (0, 1, 65535, 65536, 131070, 131071):
        assert E.stored_bound(n) == n + 5 * -(-n // 65535) + 6
