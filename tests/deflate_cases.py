"""Inputs for the audit of the device DEFLATE: the smallest at which each stage can go wrong.  Every case is
(name, data, bpp, row) — the bytes and the two distance hints given to `png.zlib_compress`.  All are built from seeded
generators or planted copies, on first use.  tests/test_deflate_tokens_cpu.py asserts, without a GPU, that each case reaches
the edge it is named after.  Test harness only."""
import numpy as np

import synth

CHUNK = 65535
_HASH_BITS = 14


def _bucket(b0, b1, b2, b3):
    return (((b0 | b1 << 8 | b2 << 16 | b3 << 24) * 2654435761) & 0xFFFFFFFF) >> (32 - _HASH_BITS)


def _noise(n, seed):
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8).tobytes()


def _noise7(n, seed):
    """Noise over 128 byte values: next to nothing to match, but 7 bits a byte, so the block is dynamic and its tokens can be read."""
    return (np.random.RandomState(seed).randint(0, 128, n) * 2 + 1).astype(np.uint8).tobytes()


def _tiny(k):
    return bytes((i % 3) * 50 + 1 for i in range(k)), 3, 0  # period 3 through the bpp hint: a match from 6 bytes on


def _repeat(block, n):
    return (block * (n // len(block) + 1))[:n]


def _substep(n):
    return _repeat(synth.lcg_bytes(300, 21).tobytes(), n), 0, 0


def _chunk(n):
    return _repeat(synth.lcg_bytes(3000, 22).tobytes(), n), 0, 0


def segment_straddle_plan():
    """[(position, length, distance)] of the planted copies: 258 and 5 bytes at positions 62, 63, 0 and 1 mod 64."""
    plan, p = [], 4096
    for length in (258, 5):
        for res in (62, 63, 0, 1):
            p += 300
            p += (res - p) % 64
            plan.append((p, length, 1500 + 8 * len(plan)))
            p += length
    return plan


def _segment_straddle():
    d = bytearray(_avoiding_noise(9000, np.random.RandomState(23), set(), fresh=set()))  # a bucket per group: the table keeps every source
    for p, length, dist in segment_straddle_plan():
        d[p:p + length] = d[p - dist:p - dist + length]
        if d[p + length] == d[p + length - dist]:
            d[p + length] ^= 0x55
    return bytes(d), 0, 0


def _avoiding_noise(n, rng, avoid, tail=(), fresh=None):
    """n bytes of noise over 128 values none of whose 4-byte groups (those reaching back into `tail` included) hashes into `avoid`; with
    `fresh`, a set, every group also gets a bucket of its own, which is added to the set."""
    out = bytearray(tail[-3:])
    skip = len(out)
    draws = rng.randint(0, 128, 4 * n + 64) * 2 + 1  # 128 byte values: the literals cost 7 bits, the block is not stored
    k = 0
    while len(out) - skip < n:
        b = int(draws[k])
        k += 1
        if len(out) >= 3:
            h = _bucket(out[-3], out[-2], out[-1], b)
            if h in avoid or (fresh is not None and h in fresh):
                continue
            if fresh is not None:
                fresh.add(h)
        out.append(b)
    return bytes(out[skip:])


WINDOW_MARKER = 400


def window_layout(dist, where):
    """-> (start of the first copy, start of the second, total length)"""
    second = CHUNK + 2000 if where == "early" else CHUNK - 200
    return second - dist, second, second + WINDOW_MARKER + 600


def _window(dist, where):
    """Noise with a 400-byte marker at two places `dist` apart.  Half of a noise stream's 4-byte groups lose their table
    entry to a later group within 11,000 positions, so the noise is drawn such that no group outside the marker falls
    into a bucket of the marker's groups, and the marker's groups have a bucket each: the table must then offer the first
    copy at every position of the second — the case tests the window, not the luck of the hash."""
    first, second, total = window_layout(dist, where)
    rng = np.random.RandomState(24)
    own = set()
    marker = _avoiding_noise(WINDOW_MARKER, rng, set(), fresh=own)
    d = bytearray(_avoiding_noise(first, rng, own))
    d += marker
    d += _avoiding_noise(second - len(d), rng, own, tail=d)
    d += marker
    d += _avoiding_noise(total - len(d), rng, own, tail=d)
    # (groups that begin in the last three bytes of a marker copy reach into noise: they were drawn against `own` too)
    return bytes(d), 0, 0


LEN3_POSITIONS = [4500 + 97 * k for k in range(40)]


def _len3(row):
    """Three bytes repeated from `row` back with a fourth that differs: a 4-byte hash cannot find them, distance 1 does not."""
    d = bytearray(_noise7(4500 + 97 * 40 + 50, 25))
    for p in LEN3_POSITIONS:
        d[p:p + 3] = d[p - row:p - row + 3]
        for q in (p - 1, p + 3):  # three bytes, not one more on either side
            if d[q] == d[q - row]:
                d[q] ^= 0x33
    return bytes(d), 0, row


def _tie_period7():
    """Period 7 with a byte broken every 211: between two breaks the hints 14 and 21 (and whatever the table offers, a
    multiple of 7) give the same length below the cap of 258, so the distance is decided by the tie rule alone."""
    d = bytearray((i % 7) * 37 & 255 for i in range(3000))
    for p in range(211, 3000, 211):
        d[p] ^= 0x80
    return bytes(d), 14, 21


def _form_tie(alphabet, n):
    """Short noise over a few byte values at a length where forms tie in bytes (found by a search over n with the reference
    sizes of deflate_reference; tests/test_deflate_tokens_cpu.py asserts the tie): 8 values, 30 bytes — fixed = dynamic = 32,
    fixed must win; 32 values, 85 bytes — stored = fixed = dynamic = 90, stored must win."""
    return bytes((np.random.RandomState(1).randint(0, alphabet, n) * 7 + 3).astype(np.uint8)), 0, 0


WIDE_FAR = 20011  # the row hint of wide_tokens: distance symbol 28, 13 extra bits


def _wide_tokens():
    """Noise literals; every dozen bytes 3 to 5 bytes copied from 1 or 3 back (found through distance 1 and the bpp hint);
    from 21,000 on, every 1,500 bytes a copy of 131 to 257 bytes from 20,011 back (found through the row hint)."""
    rng = np.random.RandomState(26)
    d = bytearray()
    next_far, far = 21000, 0
    while len(d) < 60000:
        if len(d) >= next_far:
            length = 131 + (far * 37) % 127
            for _ in range(length):
                d.append(d[-WIDE_FAR])
            d.append(d[-WIDE_FAR] ^ 0x5A)
            far += 1
            next_far = len(d) + 1500
            continue
        d += rng.randint(0, 256, int(rng.randint(8, 17))).astype(np.uint8).tobytes()
        near = 1 if rng.randint(0, 2) else 3
        for _ in range(int(rng.randint(3, 6))):
            d.append(d[-near])
    return bytes(d), 3, WIDE_FAR


DEEP_LIT_LENGTHS = [4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43]  # one length per symbol 258..274


def _deep_literals():
    """A literal/length tree that is deeper than 15 when unlimited.  The Fibonacci input of tests/test_gpu_png_encode.py
    (kept as `fibonacci_literals`) does not give one: with 22 byte values most of its 3- and 4-byte groups repeat, the
    finder turns them into matches, and what is left of the literal counts gives a tree 13 deep.  Counts the finder cannot
    disturb are those of length symbols: a first chunk of noise (stored; its counts do not matter), then a second chunk
    that consists of matches only, copied from places the table still holds — picked as in deep_distances — with the 17
    lengths above occurring 2584, 1597, ... 3, 2, 1 times.  With the end-of-block symbol's 1 that is a chain 17 deep (a
    second symbol with the count 1 would let two subtrees grow in turn, and halve the depth).  Each
    copy ends where the next begins with another byte than its source goes on with, so no match grows, and no token starts in
    the first three positions of a sub-step, whose predecessors' groups are not known when the generator gets there."""
    rng = np.random.RandomState(28)
    f = [1, 2]
    while len(f) < len(DEEP_LIT_LENGTHS):
        f.append(f[-1] + f[-2])
    pool = [l for l, c in zip(DEEP_LIT_LENGTHS, reversed(f)) for _ in range(c)]
    pool = [pool[i] for i in rng.permutation(len(pool))]
    d = bytearray(_noise(CHUNK, 29))
    latest = {}
    filled = CHUNK - 32768
    differ = None  # the byte the next copy must not begin with
    while pool:
        p = len(d)
        base = CHUNK + ((p - CHUNK) & ~1023)
        while filled < base and filled + 4 <= p:  # (the chunk's first token meets three groups that it completes itself)
            latest[_bucket(d[filled], d[filled + 1], d[filled + 2], d[filled + 3])] = filled
            filled += 1
        k = next(i for i in range(len(pool) - 1, -1, -1) if (p + pool[i] - CHUNK) % 1024 > 2 or len(pool) == 1)
        length = pool.pop(k)
        while True:
            src = int(rng.randint(max(p - 32768, 0), base - length - 1))
            if latest.get(_bucket(d[src], d[src + 1], d[src + 2], d[src + 3])) == src and d[src] != differ and d[src] != d[p - 1]:
                break
        d += d[src:src + length]
        differ = d[src + length]
    return bytes(d), 0, 0


def _fibonacci_literals():
    """The Fibonacci input of tests/test_gpu_png_encode.py: 22 byte values with Fibonacci counts, shuffled."""
    f, out = [1, 1], bytearray()
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    for sym, count in enumerate(f):
        out += bytes([sym * 11 & 255]) * count
    rng = np.random.RandomState(3)
    return bytes(np.frombuffer(bytes(out), np.uint8)[rng.permutation(len(out))]), 0, 0


DEEP_DIST_SYMBOLS = list(range(12, 30))  # 18 distance symbols with the counts 1, 1, 2, 3, ... 2584


def _deep_distances():
    """Four-byte matches whose distance symbols 12..29 occur 1, 1, 2, 3, ... 2584 times (6,764 matches, about 41 KB): an
    unlimited Huffman code over such counts is a chain 17 deep.  A match is only found where the table still holds its
    source, so each source is picked among the positions that are the latest of their bucket when the match's sub-step of
    1024 begins (the generator keeps the table the finder would have), at a distance inside the wanted symbol's range;
    the frequent symbols are the far ones, whose ranges are wide.  A noise byte that breaks the match follows each."""
    from deflate_tokens import DIST_BASE
    rng = np.random.RandomState(27)
    counts, f = {}, [1, 1]
    while len(f) < len(DEEP_DIST_SYMBOLS):
        f.append(f[-1] + f[-2])
    for s, c in zip(DEEP_DIST_SYMBOLS, f):
        counts[s] = c
    d = bytearray()
    latest, filled = {}, 0  # bucket -> latest position below `filled`, a multiple of 1024

    def fresh_byte():
        while True:
            b = int(rng.randint(0, 256))
            if not d or b != d[-1]:
                return b

    while len(d) < 3000:
        d.append(fresh_byte())
    while any(counts.values()) and len(d) < CHUNK - 8:
        p = len(d)
        base = p & ~1023
        if p - base < 3:
            d.append(fresh_byte())
            continue
        while filled < base:
            latest[_bucket(d[filled], d[filled + 1], d[filled + 2], d[filled + 3])] = filled
            filled += 1
        done = False
        for s in sorted(counts, key=lambda s: -counts[s]):
            if not counts[s]:
                break
            lo, hi = DIST_BASE[s], (DIST_BASE[s + 1] - 1 if s < 29 else 32768)
            s_lo, s_hi = max(p - hi, 0), min(p - lo, base - 1)
            if s_hi < s_lo:
                continue
            for _ in range(60):
                src = int(rng.randint(s_lo, s_hi + 1))
                o = latest.get(_bucket(d[p - 1], d[src], d[src + 1], d[src + 2]))  # what the byte before would find with this copy behind it
                if o is not None and (d[o], d[o + 1], d[o + 2]) == (d[p - 1], d[src], d[src + 1]):
                    continue
                if latest.get(_bucket(d[src], d[src + 1], d[src + 2], d[src + 3])) == src and d[src + 3] != d[src + 2]:
                    d += d[src:src + 4]
                    b = fresh_byte()
                    while b == d[src + 4]:
                        b = fresh_byte()
                    d.append(b)
                    counts[s] -= 1
                    done = True
                    break
            if done:
                break
        if not done:
            d.append(fresh_byte())
    assert not any(counts.values()), "deep_distances: matches left unplaced %r" % counts
    return bytes(d), 0, 0


ROW_W, ROW_H = 96, 64


def row_case_input(name):
    """The pixels and the fixture-style description of flat_row / gradient_row (96 x 64 RGBA, preset 0)."""
    import png_file_cases as PF
    c = dict(gen="flat" if name == "flat_row" else "gradient", w=ROW_W, h=ROW_H, color_type=3, preset=0, seed=1)
    return c, PF.make_input(c)


def _row(name):
    """The prepared stream of a 96 x 64 RGBA image at preset 0 (filter bytes and filtered rows), with the hints png.encode
    gives: 4 bytes per pixel, 96 * 4 + 1 bytes per row.  Made by the model of png.prepare (tests/png_reduce_model.py), so that
    the case exists without a GPU; the GPU audit asserts that png.prepare returns the same bytes."""
    import png_reduce_model as PM
    _, px = row_case_input(name)
    stream, layout, _ = PM.prepare(px, ROW_W, ROW_H, 3, PM.Opts.preset(0, flags=PM.NO_RAYON))
    assert layout["bytes_per_pixel"] == 4 and layout["row_bytes"] == 384
    return stream.tobytes(), 4, 385


_BUILDERS = {}
for _k in range(1, 10):
    _BUILDERS["tiny_%d" % _k] = (_tiny, _k)
for _n in (1023, 1024, 1025, 1027, 1028):
    _BUILDERS["substep_%d" % _n] = (_substep, _n)
_BUILDERS["segment_straddle"] = (_segment_straddle,)
for _n in (65534, 65535, 65536, 65538, 65539, 65535 + 1027):
    _BUILDERS["chunk_%d" % _n] = (_chunk, _n)
for _d in (32767, 32768, 32769):
    for _w in ("early", "straddle"):
        _BUILDERS["window_%d_%s" % (_d, _w)] = (_window, _d, _w)
_BUILDERS["len3_row4096"] = (_len3, 4096)
_BUILDERS["len3_row4097"] = (_len3, 4097)
_BUILDERS["tie_period7"] = (_tie_period7,)
_BUILDERS["form_tie_fixed_dynamic"] = (_form_tie, 8, 30)
_BUILDERS["form_tie_all"] = (_form_tie, 32, 85)
_BUILDERS["wide_tokens"] = (_wide_tokens,)
_BUILDERS["deep_literals"] = (_deep_literals,)
_BUILDERS["fibonacci_literals"] = (_fibonacci_literals,)
_BUILDERS["deep_distances"] = (_deep_distances,)
_BUILDERS["flat_row"] = (_row, "flat_row")
_BUILDERS["gradient_row"] = (_row, "gradient_row")

NAMES = list(_BUILDERS)
_CACHE = {}


def get(name):
    """-> (name, data, bpp, row), built once"""
    if name not in _CACHE:
        f = _BUILDERS[name]
        data, bpp, row = f[0](*f[1:])
        _CACHE[name] = (name, data, bpp, row)
    return _CACHE[name]


_MODEL = {}


def model(name):
    """-> (token lists per chunk of today's finder model, the table's offers per chunk), computed once and shared"""
    if name not in _MODEL:
        import deflate_reference as R
        _, data, bpp, row = get(name)
        seen = []
        _MODEL[name] = (R.finder_model(data, bpp, row, seen), seen)
    return _MODEL[name]
