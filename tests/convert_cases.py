"""TEST HARNESS: seeded inputs of the colour-conversion tests, and the layout of a block of images."""
import numpy as np

import convert_model as M

# every pair that exists: the four conversions, and the copy at all four bytes-per-pixel values
ALL_PAIRS = [(M.GRAY_ALPHA, M.GRAY), (M.RGBA, M.RGB), (M.RGB, M.GRAY), (M.RGBA, M.GRAY), (M.GRAY, M.GRAY), (M.GRAY_ALPHA, M.GRAY_ALPHA),
             (M.RGB, M.RGB), (M.RGBA, M.RGBA)]
BEFORE, AFTER = 0xA5, 0x3C  # the sentinels in front of and behind a destination


def pixels(w, h, ct, seed) -> np.ndarray:
    """w x h pixels of colour type ct: seeded noise over the whole byte range"""
    return np.random.default_rng([seed, w, h, ct]).integers(0, 256, w * h * M.bpp(ct), dtype=np.uint8)


def all_triples() -> np.ndarray:
    """4096 x 4096 Rgb pixels that hold every (r, g, b) once: pixel i is (i >> 16, (i >> 8) & 255, i & 255)"""
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> 16).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i & 255).astype(np.uint8)], axis=1).reshape(-1)


def block_of(shapes, seed, odd=()):
    """shapes: (w, h, ct) per image -> (records [(w, h, ct, offset)], block uint8): every image at a multiple of 16, the images
    whose index is in `odd` 1 + (index % 15) bytes behind one; the gaps hold BEFORE"""
    records, at = [], 0
    for i, (w, h, ct) in enumerate(shapes):
        if i in odd:
            at += 1 + i % 15
        records.append((w, h, ct, at))
        at = (at + w * h * M.bpp(ct) + 15) // 16 * 16
    block = np.full(at, BEFORE, np.uint8)
    for i, (w, h, ct, o) in enumerate(records):
        block[o:o + w * h * M.bpp(ct)] = pixels(w, h, ct, seed + i)
    return records, block


def destinations(records, dst_cts, odd=()):
    """The destinations of `records` in colour types dst_cts, laid out like block_of -> (records, total)"""
    out, at = [], 0
    for i, ((w, h, _, _), ct) in enumerate(zip(records, dst_cts)):
        if i in odd:
            at += 1 + (i * 7) % 15
        out.append((w, h, ct, at))
        at = (at + w * h * M.bpp(ct) + 15) // 16 * 16
    return out, at


def image_bytes(block, rec) -> np.ndarray:
    w, h, ct, o = rec
    return np.asarray(block[o:o + w * h * M.bpp(int(ct))])


def check_block(got, src_block, src_records, dst_records, fill=AFTER):
    """Every destination is the model's conversion of its source, and every byte outside the destinations still holds `fill`"""
    got = np.asarray(got)
    outside = np.ones(got.size, bool)
    for i, (s, d) in enumerate(zip(src_records, dst_records)):
        want = M.convert(image_bytes(src_block, s), int(s[2]), int(d[2]))
        have = image_bytes(got, d)
        assert have.size == want.size and np.array_equal(have, want), "image %d (%dx%d, %d -> %d) differs" % (i, s[0], s[1], int(s[2]), int(d[2]))
        outside[d[3]:d[3] + want.size] = False
    assert np.all(got[outside] == fill), "bytes outside the destinations were written"
