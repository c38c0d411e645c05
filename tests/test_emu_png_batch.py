"""CPU-only: the index arithmetic of the PNG batch kernels (png_deflate_math.h, compiled for the host): chunk -> (segment,
chunk in segment), piece -> (segment, piece), the segments' destinations.  Segment length lists are seeded random ones that
always hold the lengths around one and two chunks."""
import random

import pytest

import emu_png_batch_lib as E

EDGES = [1, 65534, 65535, 65536, 131070, 131071]


def length_lists():
    rng = random.Random(20261)
    lists = [EDGES, [1], [65535] * 5, [1] * 40]
    for _ in range(6):
        extra = [rng.choice([rng.randint(1, 300), rng.randint(60000, 140000), rng.randint(250000, 600000), 262144 - 11, 4096, 4090])
                 for _ in range(rng.randint(1, 30))]
        both = EDGES + extra
        rng.shuffle(both)
        lists.append(both)
    return lists


LISTS = length_lists()


@pytest.mark.parametrize("lens", LISTS, ids=["list%d" % i for i in range(len(LISTS))])
def test_chunk_map_is_a_bijection_and_windows_stay_inside(lens):
    L, t, n = E.lib(), E.layout(lens), len(lens)
    want = [(s, c) for s in range(n) for c in range(-(-lens[s] // E.CHUNK))]
    assert t[n].first_chunk == len(want) and t[0].first_chunk == 0
    got = []
    for g in range(t[n].first_chunk):
        s = L.emu_seg_of_chunk(t, n, g)
        c = g - t[s].first_chunk
        got.append((s, c))
        c0, wstart, nbytes, last = E.chunk_span(lens[s], c)
        assert c0 == c * E.CHUNK and 1 <= nbytes <= E.CHUNK and c0 + nbytes <= lens[s]
        assert last == (c0 + nbytes == lens[s]) == (g + 1 == t[s + 1].first_chunk)
        assert 0 <= wstart <= c0 and c0 - wstart == min(c0, E.WINDOW)  # the window: 32 KiB, never in front of the segment
        first, end = t[s].src + wstart, t[s].src + c0 + nbytes  # ... in the launch's bytes: inside [src, src + len)
        assert t[s].src <= first and end <= t[s].src + t[s].len
    assert got == want  # onto every (segment, chunk), each once, in order
    assert sum(E.chunk_span(lens[s], c)[2] for s, c in want) == sum(lens)


@pytest.mark.parametrize("lens", LISTS, ids=["list%d" % i for i in range(len(LISTS))])
def test_destinations_are_aligned_and_disjoint(lens):
    L, t, n = E.lib(), E.layout(lens), len(lens)
    at = 0
    for s in range(n):
        assert (t[s].src, t[s].len) == (sum(lens[:s]), lens[s])
        bound = lens[s] + 5 * (-(-lens[s] // 65535)) + 6
        assert L.emu_stored_bound(lens[s]) == bound
        room = L.emu_seg_framed_size(bound)
        assert room == bound + 12 * (-(-bound // E.IDAT))
        assert t[s].dst % E.ALIGN == 0 and t[s].dst >= at, "segment %d starts inside the one before" % s
        at = t[s].dst + room
        assert t[s + 1].dst >= at and t[s + 1].dst - t[s].dst == L.emu_seg_dst_bytes(lens[s])
        # the first body byte of a segment is 8 behind its start: word aligned, so words of the stream at multiples of 4 are aligned
        assert (t[s].dst + L.emu_seg_framed_offset(0)) % 4 == 0
    assert t[n].dst >= at


@pytest.mark.parametrize("lens", LISTS, ids=["list%d" % i for i in range(len(LISTS))])
def test_piece_map_covers_every_byte_once(lens):
    L, t, n = E.lib(), E.layout(lens), len(lens)
    rng = random.Random(sum(lens))
    # every segment's real stream is somewhere between its smallest possible and its bound
    streams = [rng.choice([L.emu_stored_bound(x), 2 + 1 + 4, rng.randint(7, L.emu_stored_bound(x))]) for x in lens]
    covered = [0] * n
    seen = set()
    for g in range(t[n].first_piece):
        s = L.emu_seg_of_piece(t, n, g)
        p = g - t[s].first_piece
        assert t[s].first_piece <= g < t[s + 1].first_piece and (s, p) not in seen
        seen.add((s, p))
        s0, nbytes = E.piece_span(streams[s], p)
        assert s0 == p * E.PIECE
        if nbytes == 0:
            assert s0 >= streams[s]  # behind the stream's end: no value is written
            continue
        assert s0 == covered[s], "pieces of segment %d leave a gap or overlap" % s
        assert s0 // E.IDAT == (s0 + nbytes - 1) // E.IDAT, "a piece crosses an IDAT boundary"
        assert L.emu_seg_framed_offset(s0) == s0 + 8 + 12 * (s0 // E.IDAT)
        covered[s] += nbytes
    assert covered == streams
    assert len(seen) == t[n].first_piece == sum(-(-L.emu_stored_bound(x) // E.PIECE) for x in lens)


def test_layout_refuses_more_chunks_than_fit():
    import ctypes as C
    n = 3
    table = (E.Segment * (n + 1))()
    assert E.lib().emu_seg_layout((C.c_uint64 * n)(1 << 46, 1 << 46, 1 << 46), n, table) == 0
