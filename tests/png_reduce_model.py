"""Independent model of the reference's PNG reductions, written from its text (src/png/mod.rs:513-568, :633-1120,
src/png/bit_depth.rs) in numpy: maybe_reduce_color_type (palette in modified-Zeng order, colour type, bit depth),
maybe_optimize_alpha, then the row filters through the PNG oracle (oracle/pixo_png_oracle.c).  Test harness only.

The oracle applies the "<= 4096 pixels -> Sub" rule to the width it is given; for packed rows that is row_bytes, not
the pixel width the reference uses (filter.rs:77).  The model resolves the rule itself from the pixel area and, where
the oracle would still apply it, appends dummy rows below the image (every strategy only looks upwards)."""
import zlib

import numpy as np

import oracle_lib as O

BPP = {0: 1, 1: 2, 2: 3, 3: 4}
PNG_CT = {0: 0, 1: 4, 2: 2, 3: 6}
NO_RAYON = 1


class Opts:
    def __init__(self, filter_strategy=O.S_ADAPTIVE_FAST, optimize_alpha=False, reduce_color_type=False, reduce_palette=False, flags=0):
        self.filter_strategy, self.optimize_alpha = filter_strategy, optimize_alpha
        self.reduce_color_type, self.reduce_palette, self.flags = reduce_color_type, reduce_palette, flags

    @classmethod
    def preset(cls, p, flags=0):
        if p == 0:
            return cls(flags=flags)
        return cls(O.S_BIGRAMS if p == 2 else O.S_ADAPTIVE, True, True, True, flags)


def pack_rows(samples, bits):
    """(h, w) uint8 -> (h, ceil(w * bits / 8)), MSB first, rows padded with zero bits (bit_depth.rs:105-148)."""
    if bits == 8:
        return samples.copy()
    h, w = samples.shape
    per = 8 // bits
    padded = np.zeros((h, (w + per - 1) // per * per), np.uint8)
    padded[:, :w] = samples & ((1 << bits) - 1)
    g = padded.reshape(h, -1, per).astype(np.uint32)
    out = np.zeros(g.shape[:2], np.uint32)
    for k in range(per):
        out = (out << bits) | g[:, :, k]
    return out.astype(np.uint8)


def statistics(indexed, n):
    """Histogram and co-occurrence matrix (mod.rs:940-977) of an (h, w) index image."""
    counts = np.bincount(indexed.reshape(-1), minlength=n).astype(np.uint64)
    m = np.zeros((n, n), np.uint64)
    for a, b in ((indexed[:, :-1], indexed[:, 1:]), (indexed[:-1, :], indexed[1:, :])):
        pair = np.bincount(a.reshape(-1).astype(np.int64) * n + b.reshape(-1), minlength=n * n).reshape(n, n).astype(np.uint64)
        m += pair + pair.T
    return (counts & 0xFFFFFFFF).astype(np.uint32), (m & 0xFFFFFFFF).astype(np.uint32)


def palette_order(counts, m, info=None):
    """optimize_palette_order on the statistics: order[k] = sorted-key index of final entry k."""
    n = len(counts)
    if n <= 2:
        return list(range(n))
    m = [[int(v) for v in row] for row in m]
    edges = [((j, i), m[i][j]) for i in range(n) for j in range(i) if m[i][j] > 0]
    if not edges:
        return list(range(n))
    edges.sort(key=lambda e: -e[1])  # stable
    remap = [edges[0][0][0], edges[0][0][1]]
    sums, best_pos, best = [], 0, (0, 0)
    for i in range(n):
        if i in remap:
            continue
        s = (m[i][remap[0]] + m[i][remap[1]]) & 0xFFFFFFFF
        if s > best[1]:
            best_pos, best = len(sums), (i, s)
        sums.append([i, s])
    while sums:
        bi = best[0]
        placed = n - len(sums)
        delta = sum((placed - 1 - 2 * i) * m[bi][idx] for i, idx in enumerate(remap))
        if delta > 0:
            remap.insert(0, bi)
        else:
            remap.append(bi)
        sums[best_pos] = sums[-1]
        sums.pop()
        best_pos, best = 0, (0, 0)
        for i, s in enumerate(sums):
            s[1] = (s[1] + m[bi][s[0]]) & 0xFFFFFFFF
            if s[1] > best[1]:
                best_pos, best = i, (s[0], s[1])
    total = int(sum(int(c) for c in counts)) & 0xFFFFFFFF
    popular, pc = remap[0], int(counts[remap[0]])
    for idx in remap:  # max_by_key: the last maximum
        if int(counts[idx]) >= pc:
            popular, pc = idx, int(counts[idx])
    branch = "skip"
    if pc >= ((total * 3) & 0xFFFFFFFF) // 20:
        pos = remap.index(popular)
        if pos >= len(remap) // 2:
            remap.reverse()
            k = (pos + 1) % len(remap)
            remap = remap[len(remap) - k:] + remap[:len(remap) - k]
            branch = "back"
        else:
            remap = remap[pos:] + remap[:pos]
            branch = "front"
    if info is not None:
        info["popular"] = branch
    return remap


def reduce(px, w, h, ct, o, info=None):
    """-> dict(rows (h, row_bytes) uint8, color_type_byte, bit_depth, bytes_per_pixel, palette or None)."""
    spp = BPP[ct]
    img = np.ascontiguousarray(px, np.uint8).reshape(h, w, spp)
    res = dict(rows=img.reshape(h, w * spp), color_type_byte=PNG_CT[ct], bit_depth=8, bytes_per_pixel=spp, palette=None, eff=ct)
    if ct == 0 and o.reduce_color_type:
        return res  # mod.rs:691-700
    if o.reduce_palette and ct in (2, 3):
        v = img.astype(np.uint32)
        keys = (v[:, :, 0] << 24) | (v[:, :, 1] << 16) | (v[:, :, 2] << 8) | (v[:, :, 3] if ct == 3 else 255)
        uniq = np.unique(keys)
        if len(uniq) <= 256:
            n = len(uniq)
            indexed = np.searchsorted(uniq, keys).astype(np.uint8)
            counts, m = statistics(indexed, n)
            order = palette_order(counts, m, info)
            bmap = np.zeros(256, np.uint8)
            bmap[np.array(order)] = np.arange(n, dtype=np.uint8)
            bits = 1 if n <= 2 else 2 if n <= 4 else 4 if n <= 16 else 8
            pal = [(int(k) >> 24, (int(k) >> 16) & 255, (int(k) >> 8) & 255, int(k) & 255) for k in uniq[np.array(order)]]
            res.update(rows=pack_rows(bmap[indexed], bits), color_type_byte=3, bit_depth=bits, bytes_per_pixel=1, palette=pal, eff=2,
                       counts=counts, matrix=m, order=order)
            return res
    if not o.reduce_color_type or ct in (0, 1):
        return res

    def to_gray():
        g = img[:, :, 0]
        mx = int(g.max())
        bits = 1 if mx <= 1 else 2 if mx <= 3 else 4 if mx <= 15 else 8
        res.update(rows=pack_rows(g, bits), color_type_byte=0, bit_depth=bits, bytes_per_pixel=1, eff=0)
        return res
    gray = bool(((img[:, :, 0] == img[:, :, 1]) & (img[:, :, 1] == img[:, :, 2])).all())
    if ct == 2:
        return to_gray() if gray else res
    opaque = bool((img[:, :, 3] == 255).all())
    if opaque and gray:
        return to_gray()
    if opaque:
        res.update(rows=np.ascontiguousarray(img[:, :, :3]).reshape(h, w * 3), color_type_byte=2, bytes_per_pixel=3, eff=2)
    elif gray:
        res.update(rows=np.ascontiguousarray(img[:, :, [0, 3]]).reshape(h, w * 2), color_type_byte=4, bytes_per_pixel=2, eff=1)
    return res


def optimize_alpha(res, o):
    if not o.optimize_alpha or res["eff"] not in (1, 3):
        return
    spp = BPP[res["eff"]]
    rows = res["rows"]
    p = rows.reshape(rows.shape[0], -1, spp).copy()
    p[:, :, :spp - 1][p[:, :, spp - 1] == 0] = 0
    res["rows"] = p.reshape(rows.shape)


def filter_rows(rows, w, h, bpp, strategy, flags):
    """apply_filters_with_row_bytes: the area rule on PIXELS, the stateful AdaptiveFast where the reference runs it."""
    row_bytes = rows.shape[1]
    adaptive = strategy in (O.S_ADAPTIVE, O.S_ADAPTIVE_FAST, O.S_BIGRAMS)
    if adaptive and w * h <= 4096:
        strategy, adaptive = O.S_SUB, False
    stateful = strategy == O.S_ADAPTIVE_FAST and bool((flags & NO_RAYON) or h <= 32)
    f_w = row_bytes // bpp
    assert f_w * bpp == row_bytes
    hh = h
    if adaptive and f_w * h <= 4096:  # the oracle would still say Sub: make its area pass 4096 with dummy rows
        hh = 4096 // f_w + 1
        rows = np.vstack([rows, np.zeros((hh - h, row_bytes), np.uint8)])
    flt, _ = O.png_filter(np.ascontiguousarray(rows).reshape(-1), f_w, hh, bpp, strategy, stateful)
    flt = flt[:h * (row_bytes + 1)]
    return flt, zlib.adler32(flt.tobytes()) & 0xFFFFFFFF


def prepare(px, w, h, ct, o, info=None):
    """-> (stream uint8 array, layout dict, adler32)"""
    res = reduce(px, w, h, ct, o, info)
    optimize_alpha(res, o)
    flt, adler = filter_rows(res["rows"], w, h, res["bytes_per_pixel"], o.filter_strategy, o.flags)
    pal = res["palette"]
    layout = dict(color_type_byte=res["color_type_byte"], bit_depth=res["bit_depth"], bytes_per_pixel=res["bytes_per_pixel"],
                  row_bytes=res["rows"].shape[1], palette=pal or [], has_trns=bool(pal) and any(p[3] != 255 for p in pal))
    return flt, layout, adler


def layout_of(lay):
    """A pixo_amd.png.PngLayout as the dict this model returns."""
    return dict(color_type_byte=lay.color_type_byte, bit_depth=lay.bit_depth, bytes_per_pixel=lay.bytes_per_pixel,
                row_bytes=lay.row_bytes, palette=[tuple(p) for p in lay.palette], has_trns=lay.has_trns)
