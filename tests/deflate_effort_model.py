"""The high effort of the device DEFLATE (pixo_amd/csrc/png_deflate.hip, steps 1a to 1c) restated as a plain
sequential program, per chunk: links through earlier occurrences of a 4-byte hash, built in sub-steps whose look-ups
come before their inserts; at every position the distances 1, bpp, up to `probes` entries along the links, row; a
one-step lazy walk.  Tokens are those of deflate_tokens.  Uses the byte loop, the hash and the constants of
deflate_reference; imports nothing of this library.  Test harness only."""
import numpy as np

import deflate_reference as R
from deflate_reference import CHUNK, HASH_BITS, MAX_MATCH, MIN_MATCH, WINDOW, _agree, hash4_all


def heads_seen(h_all, total_len, c0, n, substep):
    """-> for every position of [wstart, c0 + n), counted from wstart: the stream position of the head its look-up saw,
    -1 for none.  The window and the chunk are walked in sub-steps of `substep` positions from wstart; the head of a
    hash is its latest position in earlier sub-steps; a window position takes part while four bytes of the stream are
    left, a chunk position while four bytes of the chunk are."""
    wstart = max(c0 - WINDOW, 0)
    total = c0 - wstart + n
    head = np.full(1 << HASH_BITS, -1, np.int64)
    seen = np.full(total, -1, np.int64)
    for s0 in range(0, total, substep):
        a = wstart + np.arange(s0, min(s0 + substep, total))
        a = a[np.where(a < c0, a + 4 <= total_len, a - c0 + 4 <= n)]
        if len(a):
            hs = h_all[a]
            seen[a - wstart] = head[hs]  # every look-up of the sub-step comes before its inserts
            np.maximum.at(head, hs, a)
    return seen


def effort_model(data, bpp, row, substep, probes, trace=None):
    """-> one token list per chunk of 65,535 bytes.  `trace`, a list: receives per chunk a dict with `best` ((length,
    distance) kept at every position, (0, 0): none), `chain` (per position the (distance, length) of every chain entry
    looked at — length None where it was skipped because the best length was the cap), `beyond` (per position the distance
    of the entry at which the chain stopped for being farther than the window, 0: it did not) and `deferred` (positions
    given up as a literal for a longer match at the next)."""
    data = bytes(data)
    total_len = len(data)
    h_all = hash4_all(data)
    out = []
    for c0 in range(0, total_len, CHUNK):
        n = min(CHUNK, total_len - c0)
        wstart = max(c0 - WINDOW, 0)
        seen = heads_seen(h_all, total_len, c0, n, substep)
        best = [(0, 0)] * n
        chains, beyond = [()] * n, [0] * n
        for p in range(n):
            a = c0 + p
            limit = min(n - p, MAX_MATCH)
            if limit < MIN_MATCH:
                continue
            bl = bd = 0
            tried = []

            def attempt(d):
                nonlocal bl, bd
                if d == 0 or d > WINDOW or d > a or bl == limit:
                    return None
                l = _agree(data, a, a - d, limit)
                if l > bl or (l == bl and d < bd):
                    bl, bd = l, d
                return l

            attempt(1)
            if bpp > 1:
                attempt(bpp)
            e = int(seen[a - wstart])
            for _ in range(probes):
                if e < 0:
                    break
                if a - e > WINDOW:
                    beyond[p] = a - e
                    break
                tried.append((a - e, attempt(a - e)))
                e = int(seen[e - wstart])
            if row > 1 and row != bpp:
                attempt(row)
            chains[p] = tuple(tried)
            if bl < MIN_MATCH or (bl == MIN_MATCH and bd > 4096):
                continue
            best[p] = (bl, bd)
        tokens, deferred, p = [], [], 0
        while p < n:
            l, d = best[p]
            if p + 1 < n and best[p + 1][0] > l:
                if l:
                    deferred.append(p)
                l = 0
            if l:
                tokens.append((c0 + p, l, d))
                p += l
            else:
                tokens.append((c0 + p, data[c0 + p]))
                p += 1
        out.append(tokens)
        if trace is not None:
            trace.append(dict(best=best, chain=chains, beyond=beyond, deferred=deferred, seen=seen, wstart=wstart))
    return out


def estimated_bytes(tokens):
    """Bytes of a block holding these tokens, from the cost functions of deflate_reference: optimal code costs + extra
    bits + 300 bits for a dynamic header, or the fixed form where that is smaller."""
    lit, dist, extra = R.histograms(tokens)
    dynamic = R.huffman_cost(lit)[0] + R.huffman_cost(dist)[0] + extra + 300
    return (min(dynamic, R.fixed_cost(tokens)) + 7) // 8
