"""Deterministic PNG files for the decoder's tests, assembled here from `synth` bytes with zlib and struct so that the filter
of every row can be chosen freely (mixes an encoder would never write included), and a builder of broken files.  The model's
reading of a file is computed once per file, shared and never changed.  Test harness only."""
import hashlib
import struct
import zlib

import numpy as np

import png_decode_model as M
import synth

GRAY, RGB, INDEXED, GRAY_ALPHA, RGBA = M.GRAY, M.RGB, M.INDEXED, M.GRAY_ALPHA, M.RGBA
COMBOS = [(ct, d) for ct in (GRAY, RGB, INDEXED, GRAY_ALPHA, RGBA) for d in M.VALID_DEPTHS[ct]]  # the 15 legal pairs
assert len(COMBOS) == 15


def chunk(ctype, body, crc=None):
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", zlib.crc32(ctype + body) if crc is None else crc)


def ihdr(w, h, depth, ct, comp=0, flt=0, lace=0):
    return struct.pack(">IIBBBBB", w, h, depth, ct, comp, flt, lace)


def paeth(a, b, c):
    return M.paeth(a, b, c)


def filter_rows(raw, h, rb, bpp, filters):
    """The forward filters: raw rows -> the stream with filter byte filters[y] in front of row y (a byte above 4 is stored with
    the row unfiltered)"""
    out, prev = bytearray(), bytes(rb)
    for y in range(h):
        row, ft = raw[y * rb:(y + 1) * rb], filters[y]
        if 1 <= ft <= 4:
            r = np.frombuffer(row, np.uint8).astype(np.int32)
            p = np.frombuffer(prev, np.uint8).astype(np.int32)
            a = np.concatenate([np.zeros(min(bpp, rb), np.int32), r[:-bpp]])[:rb] if rb > bpp else np.zeros(rb, np.int32)
            c = np.concatenate([np.zeros(min(bpp, rb), np.int32), p[:-bpp]])[:rb] if rb > bpp else np.zeros(rb, np.int32)
            if ft == 1:
                pred = a
            elif ft == 2:
                pred = p
            elif ft == 3:
                pred = (a + p) >> 1
            else:
                pq = a + p - c
                pa, pb, pc = np.abs(pq - a), np.abs(pq - p), np.abs(pq - c)
                pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, p, c))
            row_f = ((r - pred) & 255).astype(np.uint8).tobytes()
        else:
            row_f = row
        out += bytes([ft]) + row_f
        prev = row
    return bytes(out)


def palette_of(n, seed):
    return synth.lcg_bytes(3 * n, seed).tobytes()


def make(w, h, ct, depth, filters=None, seed=1, plte_entries=None, trns=None, level=6, idat_split=None, no_plte=False, extra=b""):
    """A well-formed file (unless no_plte / a filter byte above 4 says otherwise).  filters: per-row list, an int for every row,
    or None for rows cycling 0-4.  plte_entries: fewer than 2^depth leaves indices beyond the palette."""
    rb, bpp = M.row_bytes(ct, depth, w), M.filter_unit(ct, depth)
    raw = synth.lcg_bytes(h * rb, seed).tobytes()
    if filters is None:
        filters = [y % 5 for y in range(h)]
    elif isinstance(filters, int):
        filters = [filters] * h
    stream = filter_rows(raw, h, rb, bpp, filters)
    z = zlib.compress(stream, level)
    out = M.SIGNATURE + chunk(b"IHDR", ihdr(w, h, depth, ct)) + extra
    if ct == INDEXED and not no_plte:
        out += chunk(b"PLTE", palette_of((1 << depth) if plte_entries is None else plte_entries, seed + 100))
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    parts = [z] if not idat_split else [z[i:i + idat_split] for i in range(0, len(z), idat_split)]
    for p in parts:
        out += chunk(b"IDAT", p)
    return out + chunk(b"IEND", b"")


def random_filters(h, seed):
    return [int(v) % 5 for v in synth.lcg_bytes(h, seed)]


_MODEL = {}


def model(png):
    """The model's reading of a file: (w, h, pixels, colour type), or the DecodeError it raises; computed once per file"""
    k = hashlib.sha256(png).digest()
    if k not in _MODEL:
        try:
            _MODEL[k] = M.decode_png(png)
        except M.DecodeError as e:
            _MODEL[k] = e
    return _MODEL[k]


def trns_for(ct, depth, seed):
    """Palette files alternate: no tRNS, a short tRNS with alpha, an all-255 tRNS"""
    if ct != INDEXED:
        return None
    return [None, bytes([0, 128]), bytes([255, 255])][(depth + seed) % 3]


SIZES = [(1, 1), (1, 70), (70, 1), (67, 65), (129, 130)]


def shape_cases(pass_rows):
    """Every colour type x legal depth at every size (and the one that crosses two pass boundaries): (name, file)"""
    for (w, h) in SIZES + [(33, 2 * pass_rows + 3)]:
        for i, (ct, d) in enumerate(COMBOS):
            kw = dict(trns=trns_for(ct, d, w), plte_entries=(max((1 << d) - 1, 1) if d < 8 else 200) if ct == INDEXED else None)
            # the tall case: one run of Paeth / Average / Up rows under a Sub row, so that it crosses both pass boundaries
            filters = [1] + [2 + (y % 3) for y in range(1, h)] if h == 2 * pass_rows + 3 else None
            yield "c%d_d%d_%dx%d" % (ct, d, w, h), make(w, h, ct, d, filters=filters, seed=7 + i, **kw)


def layout_cases():
    """Filter layouts on 67x131 RGB and RGBA"""
    w, h = 67, 131
    for ct in (RGB, RGBA):
        for ft in range(5):
            yield "c%d_all%d" % (ct, ft), make(w, h, ct, 8, filters=ft, seed=20 + ft)
        yield "c%d_cycle" % ct, make(w, h, ct, 8, seed=30)
        yield "c%d_random" % ct, make(w, h, ct, 8, filters=random_filters(h, 31), seed=31)
        f = [4] * h
        f[64], f[65] = 1, 0
        yield "c%d_paeth_sub64_none65" % ct, make(w, h, ct, 8, filters=f, seed=32)
        f = [4] * h
        f[h - 1] = 0
        yield "c%d_start_on_last_row" % ct, make(w, h, ct, 8, filters=f, seed=33)
        for ft in (2, 3, 4):
            yield "c%d_row0_%d" % (ct, ft), make(w, h, ct, 8, filters=[ft] + [y % 5 for y in range(1, h)], seed=34 + ft)


# ---- broken files -----------------------------------------------------------------------------------------------------------
def _good(ct=RGB, depth=8, w=5, h=4, **kw):
    return make(w, h, ct, depth, seed=3, **kw)


def _with_ihdr(body, crc=None, rest=None):
    idat = chunk(b"IDAT", zlib.compress(b"\0" * 8))
    return M.SIGNATURE + chunk(b"IHDR", body, crc) + (idat if rest is None else rest) + chunk(b"IEND", b"")


def _bad_crc(png, ctype):
    at = png.index(ctype) - 4
    n = struct.unpack(">I", png[at:at + 4])[0]
    crc_at = at + 8 + n
    return png[:crc_at] + bytes([png[crc_at] ^ 1]) + png[crc_at + 1:]


def broken_cases():
    """(name, file) whose refusal is decided by the walk and its checks: the model raises for every one of them"""
    good = _good()
    pal = make(5, 4, INDEXED, 8, seed=3, trns=bytes([1, 2]))
    yield "bad_signature", b"\x89PNG\r\n\x1a\x0b" + good[8:]
    yield "short_signature", good[:7]
    yield "truncated_chunk", M.SIGNATURE + chunk(b"IHDR", ihdr(1, 1, 8, 0)) + struct.pack(">I", 100) + b"IDAT" + bytes(20)
    for t in (b"IHDR", b"IDAT", b"IEND"):
        yield "crc_" + t.decode(), _bad_crc(good, t)
    for t in (b"PLTE", b"tRNS"):
        yield "crc_" + t.decode(), _bad_crc(pal, t)
    yield "crc_unknown_chunk", _bad_crc(make(5, 4, RGB, 8, seed=3, extra=chunk(b"gAMA", b"\0\1\x86\xa0")), b"gAMA")
    yield "crc_non_utf8_type", M.SIGNATURE + chunk(b"IHDR", ihdr(1, 1, 8, 0)) + chunk(b"ab\xff\xc3", b"", crc=5) + chunk(b"IEND", b"")
    yield "ihdr_12_bytes", _with_ihdr(ihdr(1, 1, 8, 0)[:12])
    yield "plte_4_bytes", M.SIGNATURE + chunk(b"IHDR", ihdr(1, 1, 8, 3)) + chunk(b"PLTE", b"\1\2\3\4") + chunk(b"IDAT", b"x") + chunk(b"IEND", b"")
    yield "missing_iend", good[:-12]
    yield "missing_ihdr", M.SIGNATURE + chunk(b"IEND", b"")
    yield "zero_width", _with_ihdr(ihdr(0, 1, 8, 0))
    yield "zero_height", _with_ihdr(ihdr(1, 0, 8, 0))
    yield "width_above_2_24", _with_ihdr(ihdr((1 << 24) + 1, 1, 8, 0))
    yield "compression_1", _with_ihdr(ihdr(1, 1, 8, 0, comp=1))
    yield "filter_method_1", _with_ihdr(ihdr(1, 1, 8, 0, flt=1))
    yield "interlace_1", _with_ihdr(ihdr(1, 1, 8, 0, lace=1))
    yield "color_type_5", _with_ihdr(ihdr(1, 1, 8, 5))
    for ct in (GRAY, RGB, INDEXED, GRAY_ALPHA, RGBA):
        for d in (1, 2, 3, 4, 8, 16, 32):
            if d not in M.VALID_DEPTHS[ct]:
                yield "depth_%d_for_c%d" % (d, ct), _with_ihdr(ihdr(1, 1, d, ct))
    yield "no_idat", _with_ihdr(ihdr(1, 1, 8, 0), rest=b"")
    yield "empty_idat", _with_ihdr(ihdr(1, 1, 8, 0), rest=chunk(b"IDAT", b""))
    # two faults each, to pin the order: the chunk's CRC comes before its fields; interlace before bit depth
    yield "two_bad_crc_after_invalid_ihdr_field", _with_ihdr(ihdr(1, 1, 8, 0, comp=1), rest=chunk(b"IDAT", b"x", crc=1))
    yield "two_interlace_and_bad_depth", _with_ihdr(ihdr(1, 1, 3, 2, lace=1))
