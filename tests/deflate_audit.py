"""The layers of the DEFLATE audit: each takes a zlib stream as read by deflate_tokens.read_zlib and the bytes it was made
from, and checks one stage of the compressor against its plain reference in deflate_reference.  The first five hold
for any match finder; `todays_finder` pins the finder of DESIGN §4.6c.  The GPU audit (tests/test_gpu_png_deflate_tokens.py)
runs them on what the device wrote, tests/test_deflate_tokens_cpu.py on the stream assembled from the model's tokens.
Test harness only."""
import zlib

import deflate_reference as R
import deflate_tokens as T
import emu_png_deflate_lib as E

CHUNK = R.CHUNK


def chunks_of(z, data):
    """[(block, c0, n, last)] — the block of every 65,535-byte chunk.  A fixed or dynamic block that is not the last is
    followed by the empty stored block; a stored one ends on a byte boundary by itself and is followed by nothing."""
    out, i = [], 0
    count = -(-len(data) // CHUNK)
    for c in range(count):
        assert i < len(z.blocks), "layout: the stream has no block for chunk %d" % c
        out.append((z.blocks[i], c * CHUNK, min(CHUNK, len(data) - c * CHUNK), c == count - 1))
        i += 1 if (c == count - 1 or z.blocks[i].btype == T.STORED) else 2
    assert i == len(z.blocks), "layout: %d blocks for %d chunks" % (len(z.blocks), count)
    return out


def layout(z, stream, data):
    assert zlib.adler32(data) == z.adler32, "layout: the Adler-32 is not that of the input"
    assert z.data == data, "layout: the blocks do not produce the input"
    assert len(stream) == 2 + (z.end - 16 + 7) // 8 + 4, "layout: the total length is not 2 + blocks + 4"
    cs = chunks_of(z, data)
    for k, (b, c0, n, last) in enumerate(cs):
        assert b.start % 8 == 0, "layout: the block of chunk %d starts at bit %d" % (k, b.start)
        assert b.out_start == c0 and b.data == data[c0:c0 + n], "layout: the block of chunk %d does not produce its chunk's bytes" % k
        assert bool(b.final) == last, "layout: BFINAL of chunk %d" % k
        if not last and b.btype != T.STORED:
            e = z.blocks[z.blocks.index(b) + 1]
            assert e.btype == T.STORED and not e.final and e.data == b"" and e.start == b.end, "layout: no empty stored block behind chunk %d" % k
    return cs


def validity(cs, data):
    for k, (b, c0, n, last) in enumerate(cs):
        for t in b.tokens:
            assert c0 <= t[0] < c0 + n
            if len(t) == 3:
                p, l, d = t
                assert 3 <= l <= 258, "validity: length %d at %d" % (l, p)
                assert 1 <= d <= 32768 and d <= p, "validity: distance %d at %d" % (d, p)
                assert p + l <= c0 + n, "validity: the match at %d crosses the end of chunk %d" % (p, k)
                assert not (l == 3 and d > 4096), "validity: length 3 at distance %d (position %d)" % (d, p)


def maximal(cs, data):
    for b, c0, n, last in cs:
        for t in b.tokens:
            if len(t) == 3:
                p, l, d = t
                if l < 258 and p + l < c0 + n:
                    assert data[p + l] != data[p + l - d], "maximal matches: the match (%d, %d) at %d could be one longer" % (l, d, p)


def explicit(cs, data, bpp, row):
    for b, c0, n, last in cs:
        for t in b.tokens:
            el, ed = R.explicit_best(data, c0, n, t[0] - c0, bpp, row)
            if len(t) == 2:
                assert el == 0, "explicit candidates: a literal at %d, distance %d gives %d bytes" % (t[0], ed, el)
            else:
                assert t[1] >= el, "explicit candidates: (%d, %d) at %d, distance %d gives %d bytes" % (t[1], t[2], t[0], ed, el)
                assert t[1] > el or t[2] <= ed, "explicit candidates: (%d, %d) at %d, distance %d is as long" % (t[1], t[2], t[0], ed)


def tree_report(freq, lens, limit=15):
    """-> (cost, depth of the code, unlimited depth, excess over package-merge) of one tree as written"""
    cost = sum(f * l for f, l in zip(freq, lens))
    _, depth = R.huffman_cost(freq)
    return cost, max(lens), depth, cost - R.package_merge_cost(freq, limit)


def entropy(cs):
    for k, (b, c0, n, last) in enumerate(cs):
        if b.btype != T.DYNAMIC:
            continue
        lit, dist, extra = R.histograms(b.tokens)
        lit_lens = b.lit_lens + [0] * (286 - b.hlit)
        dist_lens = b.dist_lens + [0] * (30 - b.hdist)
        body = b.eob_offset + b.eob_width - b.first_token
        assert body == R.coded_bits(b.tokens, lit_lens, dist_lens), "entropy: the body bits of chunk %d are not length * frequency + extra bits" % k
        for what, freq, lens in (("literal/length", lit, lit_lens), ("distance", dist, dist_lens)):
            used = [s for s, f in enumerate(freq) if f]
            assert T.kraft(lens) == 1 << 15, "entropy: Kraft sum of the %s code of chunk %d" % (what, k)
            if len(used) < 2:  # zlib's fill: symbols 0 and / or 1 at one bit beside the only symbol in use
                only = used[0] if used else 0
                want = [0] * len(lens)
                want[only] = want[1 if only == 0 else 0] = 1
                assert lens == want, "entropy: the %s code of chunk %d for fewer than two symbols" % (what, k)
            else:
                assert all(bool(l) == bool(f) for f, l in zip(freq, lens)), "entropy: an unused %s symbol of chunk %d has a code" % (what, k)
            cost = sum(f * l for f, l in zip(freq, lens))
            best, depth = R.huffman_cost(freq)
            if depth <= 15:
                assert cost == best, "entropy: the %s code of chunk %d costs %d bits, an optimal one %d" % (what, k, cost, best)
            else:
                assert cost >= R.package_merge_cost(freq, 15)
                assert lens == [int(v) for v in E.huffman_lengths(freq, 15)], "entropy: the limited %s lengths of chunk %d are not the limiter's" % (what, k)
        assert b.hlit == 257 or b.lit_lens[-1], "entropy: HLIT of chunk %d keeps a trailing zero" % k
        assert b.hdist == 1 or b.dist_lens[-1], "entropy: HDIST of chunk %d keeps a trailing zero" % k
        assert b.hclen == 4 or b.cl_lens[T.CL_ORDER[b.hclen - 1]], "entropy: HCLEN of chunk %d keeps a trailing zero" % k


def emu_tokens(tokens):
    return [t[1] if len(t) == 2 else E.match(t[1], t[2]) for t in tokens]


def form(z, cs, data, tokens_of_stored=None):
    """The form chosen is the smallest, ties to stored, then fixed, then dynamic.  The dynamic size uses the header as read
    where the block is dynamic, else the header the host build of the header coder writes for the same tokens.  A stored
    block shows no tokens: it is judged with `tokens_of_stored` (per chunk, from the finder's model) where given, else left out."""
    for k, (b, c0, n, last) in enumerate(cs):
        chunk = data[c0:c0 + n]
        tokens = b.tokens
        if b.btype == T.STORED:
            if tokens_of_stored is None:
                continue
            tokens = tokens_of_stored[k]
        stored = R.stored_cost(n)
        fixed = R.form_bytes(R.fixed_cost(tokens), last)
        if b.btype == T.DYNAMIC:
            dynamic = R.form_bytes(b.eob_offset + b.eob_width - b.start, last)
        else:
            dynamic = len(E.block(emu_tokens(tokens), chunk, E.DYNAMIC, last)[0])
        want = R.chosen_form(stored, fixed, dynamic)
        assert b.btype == want, "form choice: chunk %d is form %d; stored %d, fixed %d, dynamic %d bytes" % (k, b.btype, stored, fixed, dynamic)
        nxt = cs[k + 1][0].start if not last else z.end
        assert (nxt - b.start + 7) // 8 == (stored, fixed, dynamic)[want], "form choice: chunk %d takes %d bytes" % (k, (nxt - b.start + 7) // 8)
        if b.btype == T.FIXED:
            assert b.eob_offset + b.eob_width - b.start == R.fixed_cost(tokens), "form choice: the fixed block of chunk %d is not coded with the fixed lengths" % k


def todays_finder(cs, data, bpp, row, model_tokens, offered):
    for k, (b, c0, n, last) in enumerate(cs):
        if b.btype == T.STORED:
            continue
        want = model_tokens[k]
        for got_t, want_t in zip(b.tokens, want):
            if got_t != want_t:
                p = min(got_t[0], want_t[0]) - c0
                raise AssertionError("today's finder: chunk %d, position %d (mod 1024: %d, mod 64: %d): the stream has %r, the model %r; the model's "
                                     "candidates at %d: %s" % (k, p, p % 1024, p % 64, got_t, want_t, want_t[0] - c0,
                                                               R.model_candidates(data, c0, n, want_t[0] - c0, bpp, row, offered[k])))
        assert len(b.tokens) == len(want), "today's finder: chunk %d has %d tokens, the model %d" % (k, len(b.tokens), len(want))


def all_layers(stream, data, bpp, row, model_tokens=None, offered=None):
    """Every layer in order on one stream -> (the stream as read, its chunks)."""
    z = T.read_zlib(stream)
    cs = layout(z, stream, data)
    validity(cs, data)
    maximal(cs, data)
    explicit(cs, data, bpp, row)
    entropy(cs)
    form(z, cs, data, model_tokens)
    if model_tokens is not None:
        todays_finder(cs, data, bpp, row, model_tokens, offered)
    return z, cs


def record(name, z, cs):
    """One line for profiles/png_deflate_audit.txt."""
    forms, tokens, deep_lit, deep_dist, widest, excess = [], 0, 0, 0, 0, 0
    for b, c0, n, last in cs:
        forms.append("SFD"[b.btype])
        tokens += len(b.tokens)
        widest = max([widest] + b.widths)
        if b.btype == T.DYNAMIC:
            lit, dist, _ = R.histograms(b.tokens)
            deep_lit, deep_dist = max([deep_lit] + b.lit_lens), max([deep_dist] + b.dist_lens)
            excess += tree_report(lit, b.lit_lens + [0] * (286 - b.hlit))[3]
            if sum(1 for f in dist if f) >= 2:
                excess += tree_report(dist, b.dist_lens + [0] * (30 - b.hdist))[3]
    return "%-24s blocks %d  forms %-3s  tokens %6d  deepest lit %2d dist %2d  widest token %2d bits  over package-merge %d bits" % (
        name, len(cs), "".join(forms), tokens, deep_lit, deep_dist, widest, excess)
