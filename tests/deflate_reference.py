"""Plain references for the stages of the device DEFLATE (pixo_amd/csrc/png_deflate.hip), one per stage, each the simplest
form of what the stage must compute: optimal code costs with a heap and with package-merge, the sizes of the three block
forms from RFC 1951, the longest match as a byte loop, the best of the explicit distances — and, kept apart at the end,
a model of today's match finder.  Tokens are those of deflate_tokens: (position, length, distance) or (position,
literal), positions counted from the start of the stream.  Imports nothing of this library.  Test harness only."""
import heapq

import numpy as np

import deflate_tokens as T

CHUNK, WINDOW, MIN_MATCH, MAX_MATCH = 65535, 32768, 3, 258


# ---- the entropy stage -----------------------------------------------------------------------------------------------------

def huffman_cost(freq):
    """-> (sum of frequency * code length of an optimal prefix code, its depth).  Ties between equal weights go to the
    shallower subtree, which gives the smallest depth an optimal code can have.  One symbol in use costs one bit per
    occurrence (DEFLATE has no zero-bit code); none costs nothing."""
    heap = [(int(f), 0) for f in freq if f]
    if not heap:
        return 0, 0
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, da = heapq.heappop(heap)
        b, db = heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


def package_merge_cost(freq, limit):
    """-> the smallest sum of frequency * code length over prefix codes with no length above `limit` (Larmore and
    Hirschberg's package-merge: the 2n - 2 cheapest items of the last of `limit` merged lists)."""
    leaves = sorted(int(f) for f in freq if f)
    n = len(leaves)
    if n == 0:
        return 0
    if n == 1:
        return leaves[0]
    assert n <= 1 << limit
    merged = leaves
    for _ in range(limit - 1):
        packages = [merged[i] + merged[i + 1] for i in range(0, len(merged) - 1, 2)]
        merged = sorted(leaves + packages)
    return sum(merged[:2 * n - 2])


def histograms(tokens):
    """-> (286 literal/length counts with the end-of-block symbol counted once, 30 distance counts, extra bits)"""
    lit, dist, extra = [0] * 286, [0] * 30, 0
    lit[256] = 1
    for t in tokens:
        if len(t) == 2:
            lit[t[1]] += 1
        else:
            s, e = T.length_symbol(t[1])
            lit[s] += 1
            extra += e
            s, e = T.distance_symbol(t[2])
            dist[s] += 1
            extra += e
    return lit, dist, extra


def coded_bits(tokens, lit_lens, dist_lens):
    """Bits of the tokens and the end-of-block symbol under the given code lengths."""
    lit, dist, extra = histograms(tokens)
    return extra + sum(f * lit_lens[s] for s, f in enumerate(lit) if f) + sum(f * dist_lens[s] for s, f in enumerate(dist) if f)


# ---- the form of a block (step 3 of the kernel): sizes in bytes of the block's slot ------------------------------------------

def fixed_cost(tokens):
    """Bits of a fixed block: the 3 header bits, the symbols in the code of RFC 1951 §3.2.6, end-of-block."""
    return 3 + coded_bits(tokens, T.FIXED_LIT, T.FIXED_DIST)


def stored_cost(n):
    """Bytes of a stored block of n bytes: header bits padded to a byte, LEN, NLEN, the bytes."""
    return n + 5


def form_bytes(bits, last):
    """Bytes a fixed or dynamic block of `bits` bits takes in the stream: the last block is padded to a byte; any other
    is followed by the empty stored block — 3 header bits, padding to a byte, 00 00 FF FF."""
    return (bits + 7) // 8 if last else (bits + 3 + 7) // 8 + 4


def chosen_form(stored, fixed, dynamic):
    """The smallest of the three sizes; ties go to stored, then fixed, then dynamic."""
    best = min(stored, fixed, dynamic)
    return T.STORED if stored == best else T.FIXED if fixed == best else T.DYNAMIC


# ---- matches -------------------------------------------------------------------------------------------------------------------

def longest(data, p, d, limit):
    """Bytes that agree at p and p - d, at most `limit`."""
    k = 0
    while k < limit and data[p + k] == data[p + k - d]:
        k += 1
    return k


def explicit_distances(bpp, row):
    """The distances tried at every position besides the table's: 1, the bytes of a pixel, the bytes of a row."""
    ds = [1]
    if bpp > 1:
        ds.append(bpp)
    if row > 1 and row != bpp:
        ds.append(row)
    return ds


def explicit_best(data, c0, n, p, bpp, row):
    """(length, distance) of the best match at position p of the chunk data[c0 : c0 + n] among the distances 1, bpp and row,
    (0, 0) if none is worth a token.  A distance counts when it is at most 32768 and does not reach before the start of
    the stream; the longer match wins, then the smaller distance; a match is at most 258 long and never passes the
    chunk's end; one shorter than 3, or of length 3 beyond distance 4096, is not taken."""
    a = c0 + p
    limit = min(n - p, MAX_MATCH)
    best = (0, 0)
    if limit < MIN_MATCH:
        return best
    for d in explicit_distances(bpp, row):
        if d > WINDOW or d > a:
            continue
        l = longest(data, a, d, limit)
        if l > best[0] or (l == best[0] and l and d < best[1]):
            best = (l, d)
    if best[0] < MIN_MATCH or (best[0] == MIN_MATCH and best[1] > 4096):
        return (0, 0)
    return best


# ================================================================================================================================
# THE MODEL OF TODAY'S FINDER.  Everything below pins the finder of DESIGN §4.6c as it is today; rewrite together with it.
# Its specification is the header comment of png_deflate.hip (step 1 and step 2).  Nothing above depends on it.
# ================================================================================================================================

HASH_BITS = 14


def hash4_all(data):
    """hash4 of the four bytes at every position a with a + 4 <= len(data)."""
    b = np.frombuffer(bytes(data), np.uint8).astype(np.uint64)
    if len(b) < 4:
        return np.zeros(0, np.int64)
    v = b[:-3] | (b[1:-2] << 8) | (b[2:-1] << 16) | (b[3:] << 24)
    return (((v * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)).astype(np.int64)


def _agree(data, a, b, limit):
    """longest(), fast: the first differing byte of two slices through one XOR of big integers."""
    if data[a] != data[b]:
        return 0
    x, y = data[a:a + limit], data[b:b + limit]
    if x == y:
        return limit
    v = int.from_bytes(x, "little") ^ int.from_bytes(y, "little")
    return ((v & -v).bit_length() - 1) >> 3


def finder_model(data, bpp, row, seen=None):
    """-> one token list per chunk of 65,535 bytes.  `seen`, a list: receives per chunk the distance the table offered at
    every position (0: nothing), for a report.

    Per chunk: a table of 2^14 entries, the latest position with the same hash4 relative to the window start (+ 1, 0:
    none); seeded from [wstart, c0) for positions a with a + 4 <= len; sub-steps of 1024 positions, whose look-ups see
    only the seeding and the inserts of earlier sub-steps; inserts (and look-ups) only for positions with p + 4 <= n;
    candidates in the order 1, bpp, table, row, each skipped once the best length is the cap; the longer wins, then the
    smaller distance; length 3 beyond 4096 is dropped; then the greedy walk from position 0."""
    data = bytes(data)
    total = len(data)
    h_all = hash4_all(data)
    out = []
    for c0 in range(0, total, CHUNK):
        n = min(CHUNK, total - c0)
        wstart = max(c0 - WINDOW, 0)
        table = np.zeros(1 << HASH_BITS, np.int64)
        hi = min(c0, len(h_all))  # positions a < c0 with a + 4 <= len
        if hi > wstart:
            np.maximum.at(table, h_all[wstart:hi], np.arange(wstart, hi) - wstart + 1)
        best = [(0, 0)] * n
        offered = np.zeros(n, np.int64)
        for base in range(0, n, 1024):
            end = min(base + 1024, n)
            hashed_end = max(min(end, n - 3), base)  # p + 4 <= n
            hs = h_all[c0 + base:c0 + hashed_end]
            cands = table[hs]  # the look-ups of the whole sub-step come before its inserts
            for p in range(base, end):
                a = c0 + p
                limit = min(n - p, MAX_MATCH)
                if limit < MIN_MATCH:
                    continue
                cand = int(cands[p - base]) if p < hashed_end else 0
                tries = [1]
                if bpp > 1:
                    tries.append(bpp)
                if cand:
                    tries.append(a - (wstart + cand - 1))
                    offered[p] = tries[-1]
                if row > 1 and row != bpp:
                    tries.append(row)
                bl = bd = 0
                for d in tries:
                    if d == 0 or d > WINDOW or d > a or bl == limit:
                        continue
                    l = _agree(data, a, a - d, limit)
                    if l > bl or (l == bl and d < bd):
                        bl, bd = l, d
                if bl < MIN_MATCH or (bl == MIN_MATCH and bd > 4096):
                    continue
                best[p] = (bl, bd)
            if hashed_end > base:
                np.maximum.at(table, hs, np.arange(c0 + base, c0 + hashed_end) - wstart + 1)
        tokens, p = [], 0
        while p < n:
            l, d = best[p]
            if l:
                tokens.append((c0 + p, l, d))
                p += l
            else:
                tokens.append((c0 + p, data[c0 + p]))
                p += 1
        out.append(tokens)
        if seen is not None:
            seen.append(offered)
    return out


def model_candidates(data, c0, n, p, bpp, row, offered):
    """The four candidates of the model at position p of a chunk as text: (name, distance, length) each."""
    a, limit = c0 + p, min(n - p, MAX_MATCH)
    parts = []
    for name, d in (("1", 1), ("bpp", bpp), ("table", int(offered[p])), ("row", row)):
        ok = 0 < d <= WINDOW and d <= a and limit >= MIN_MATCH
        parts.append("%s: d=%d len=%s" % (name, d, longest(data, a, d, limit) if ok else "-"))
    return "; ".join(parts)
