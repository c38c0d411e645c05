"""The reference's PNG lossy mode restated in stages, as src/png/mod.rs reads: gate (should_quantize_auto, :1708-1762),
histogram (:1518-1580), median cut (:1160-1333), k-means (:1346-1390), the 64^3 table (:1457-1499), the mapping and the
Floyd-Steinberg loop (:1616-1701), and what encode_into / encode_indexed_into put around the indices (:494-510, :1814-1902).
Pinned to the reference's own wasm build by tests/test_png_quantize_model.py.  Colours are keys r<<24 | g<<16 | b<<8 | a.
Test harness only."""
import numpy as np

OFF, AUTO, FORCE = 0, 1, 2
MAX_HIST = 8192


def keys_of(px, spp):
    p = np.asarray(px, np.uint8).reshape(-1, spp).astype(np.uint32)
    return (p[:, 0] << 24) | (p[:, 1] << 16) | (p[:, 2] << 8) | (p[:, 3] if spp == 4 else np.uint32(255))


def rgba(keys):
    k = np.asarray(keys, np.uint32)
    return np.stack([k >> 24, (k >> 16) & 255, (k >> 8) & 255, k & 255], axis=-1).astype(np.int64)


def gate(keys, max_colors):
    """should_quantize_auto on every pixel's key (the RGB key there has no alpha byte: the same number of distinct values)"""
    n = len(keys)
    if n == 0:
        return False
    unique = len(np.unique(keys[::max(n // 20000, 1)]))
    return max_colors < unique <= 32 * max_colors


def should_quantize(mode, spp, keys, max_colors):
    if mode == OFF or spp not in (3, 4):
        return False
    return True if mode == FORCE else gate(keys, min(max_colors, 256))


def histogram(keys):
    """-> (colours, counts).  Above 8,192 colours the most frequent stay; the reference's unstable sort leaves ties open, the
    library (and this model) break them by ascending key."""
    n = len(keys)
    stride = max(n // 50000, 1)
    colors, runs = np.unique(keys[::stride], return_counts=True)
    counts = np.minimum(runs.astype(np.uint64) * np.uint64(stride & 0xFFFFFFFF), 0xFFFFFFFF).astype(np.uint32)
    if len(colors) > MAX_HIST:
        keep = np.lexsort((colors, -counts.astype(np.int64)))[:MAX_HIST]
        colors, counts = colors[keep], counts[keep]
    return colors.astype(np.uint32), counts


def _box_score(c):
    lo, hi = c.min(axis=0), c.max(axis=0)
    channel, best = 0, 0
    for ch, weight in enumerate((2, 4, 1, 3)):
        s = int(hi[ch] - lo[ch]) * weight
        if ch == 0 or s > best:  # only a strictly greater score wins
            channel, best = ch, s
    return channel, best


def _entry(c, n):
    total = int(n.sum())
    if total == 0:
        return 255
    v = [int((c[:, ch] * n).sum()) // total for ch in range(4)]
    return (v[0] << 24) | (v[1] << 16) | (v[2] << 8) | v[3]


def median_cut(colors, counts, max_colors):
    """median_cut_palette before its k-means: a list of keys in box order"""
    if len(colors) == 0:
        return [255]
    boxes = [(rgba(colors), np.asarray(counts, np.int64))]
    while len(boxes) < max_colors:
        scores = [_box_score(c)[1] for c, _ in boxes]
        idx = max(i for i, s in enumerate(scores) if s == max(scores))  # max_by_key: the LAST maximum
        c, n = boxes[idx]
        if len(c) <= 1:
            break
        del boxes[idx]
        order = np.argsort(c[:, _box_score(c)[0]], kind="stable")
        c, n = c[order], n[order]
        total, acc = int(n.sum()), np.cumsum(n)
        split = min(int(np.argmax(acc >= total // 2)), len(c) - 2)
        boxes.append((c[:split + 1], n[:split + 1]))
        boxes.append((c[split + 1:], n[split + 1:]))
    return [_entry(c, n) for c, n in boxes]


def distances(colors4, entry4):
    """perceptual_distance_sq (:1405-1430) of an [n, 4] array of colours to one entry"""
    c, p = np.asarray(colors4, np.int32), np.asarray(entry4, np.int32)  # (every term stays below 2^28)
    d = c - p
    r_mean = (c[..., 0] + p[0]) >> 1
    return (((512 + r_mean) * d[..., 0] ** 2 + 1024 * d[..., 1] ** 2 + (767 - r_mean) * d[..., 2] ** 2) >> 8) + d[..., 3] ** 2


def nearest_all(colors4, palette):
    """nearest_palette_index for many colours: the FIRST entry at the minimum"""
    pal = rgba(palette)
    c4 = np.asarray(colors4, np.int32)
    best = np.full(c4.shape[:-1], 1 << 30, np.int32)
    for i, p in enumerate(pal):
        np.minimum(best, (distances(c4, p) << 8) | i, out=best)
    return (best & 255).astype(np.uint8)


def nearest_one(color4, pal4):
    """... for one colour against the palette as an [n, 4] array (the distance is symmetric in its arguments)"""
    return int(np.argmin((distances(pal4, color4).astype(np.int64) << 8) | np.arange(len(pal4))))


def kmeans(palette, colors, counts, rounds=2):
    pal, c4, n = list(palette), rgba(colors), np.asarray(counts, np.int64)
    for _ in range(rounds):
        assign = nearest_all(c4, pal)
        for i in range(len(pal)):
            m = assign == i
            total = int(n[m].sum())
            if total:
                v = [int((c4[m, ch] * n[m]).sum()) // total for ch in range(4)]
                pal[i] = (v[0] << 24) | (v[1] << 16) | (v[2] << 8) | v[3]
    return pal


def expand6(v):
    return (v << 2) | (v >> 4)


def build_lut(palette):
    cell = np.arange(64 ** 3, dtype=np.int64)
    c4 = np.stack([expand6(cell >> 12), expand6((cell >> 6) & 63), expand6(cell & 63), np.full_like(cell, 255)], axis=-1)
    return nearest_all(c4, palette)


def lookup_all(px4, lut, palette):
    """PaletteLut::lookup for an [n, 4] array: the table for opaque colours, the search for the rest"""
    p = np.asarray(px4, np.int64)
    out = lut[((p[:, 0] >> 2) << 12) | ((p[:, 1] >> 2) << 6) | (p[:, 2] >> 2)].copy()
    other = p[:, 3] != 255
    if other.any():
        out[other] = nearest_all(p[other], palette)
    return out


def dither(px4, w, h, lut, palette):
    """The Floyd-Steinberg loop in its exact integer form: errors in sixteenths.  (The reference's f32 accumulators only ever
    hold multiples of 1/16 below 2^12; test_png_quantize_model.py runs this against the wasm's output.)"""
    pal4 = rgba(palette).astype(np.int32)
    pal, searched = pal4[:, :3].tolist(), {}
    lut_l, px = lut.tolist(), np.asarray(px4, np.int64).reshape(h, w, 4).tolist()
    out = np.empty((h, w), np.uint8)
    below = [[0, 0, 0] for _ in range(w + 2)]  # what the row above diffused into column x, at [x + 1]
    for y in range(h):
        nxt = [[0, 0, 0] for _ in range(w + 2)]
        right = [0, 0, 0]
        row = px[y]
        for x in range(w):
            r, g, b, a = row[x]
            inc = below[x + 1]
            adj = []
            for ch, c in enumerate((r, g, b)):
                t = 16 * c + inc[ch] + right[ch]
                adj.append(0 if t < 0 else min(t >> 4, 255))
            if a == 255:
                idx = lut_l[((adj[0] >> 2) << 12) | ((adj[1] >> 2) << 6) | (adj[2] >> 2)]
            else:
                k = (adj[0], adj[1], adj[2], a)
                if k not in searched:
                    searched[k] = nearest_one(k, pal4)
                idx = searched[k]
            out[y, x] = idx
            p = pal[idx]
            for ch in range(3):
                e = adj[ch] - p[ch]
                right[ch] = 7 * e
                nxt[x][ch] += 3 * e
                nxt[x + 1][ch] += 5 * e
                nxt[x + 2][ch] += e
        below = nxt
    return out.reshape(-1)


def quantize(px, w, h, spp, max_colors, dithering):
    """quantize_image: -> (palette keys, indices, stage record)"""
    max_colors = min(max_colors, 256)
    keys = keys_of(px, spp)
    colors, counts = histogram(keys)
    px4 = rgba(keys)
    if len(colors) <= max_colors:  # the early out: exact lookup, the search for colours the sampling missed
        palette = [int(c) for c in colors]
        return palette, nearest_all(px4, palette), dict(colors=colors, counts=counts, early_out=True)
    cut = median_cut(colors, counts, max_colors)
    palette = kmeans(cut, colors, counts)
    lut = build_lut(palette)
    idx = dither(px4, w, h, lut, palette) if dithering else lookup_all(px4, lut, palette)
    return palette, idx, dict(colors=colors, counts=counts, early_out=False, cut=cut, lut=lut)


def trns_len(palette):
    """maybe_trim_transparency: alphas up to the last that is not 255 (0: no tRNS)"""
    alphas = [p & 255 for p in palette]
    return max([i + 1 for i, a in enumerate(alphas) if a != 255], default=0)


def indexed_strategy(strategy):
    """encode_indexed_into (:1866-1874): Adaptive 6, AdaptiveFast 7, MinSum 5 and Bigrams 8 become None"""
    return 0 if strategy in (5, 6, 7, 8) else strategy


def indexed_stream(indices, w, h, strategy=0):
    """The filtered stream of the index image for None (0) and Sub (1), bpp = 1"""
    rows = np.asarray(indices, np.uint8).reshape(h, w)
    if strategy == 1:
        rows = np.concatenate([rows[:, :1], rows[:, 1:] - rows[:, :-1]], axis=1)
    else:
        assert strategy == 0
    return np.concatenate([np.full((h, 1), strategy, np.uint8), rows], axis=1).tobytes()


def chunks_of(palette, w, h):
    """[(type, body)] of the indexed file's chunks other than IDAT"""
    import struct
    out = [("IHDR", struct.pack(">IIBBBBB", w, h, 8, 3, 0, 0, 0)), ("PLTE", b"".join(bytes([p >> 24, (p >> 16) & 255, (p >> 8) & 255]) for p in palette))]
    t = trns_len(palette)
    if t:
        out.append(("tRNS", bytes(p & 255 for p in palette[:t])))
    return out + [("IEND", b"")]
