"""TEST HARNESS: the arithmetic cases of JPEG decode, written at test time by tests/jpeg_write.py (nothing committed): the IDCT's
64 basis functions one at a time at the edge of the region jpeg_decode_math.h's header claims, dense seeded blocks near its
32-bit bound, committed files with their quantisation tables scaled up, the colour conversion over its input space and the two
fancy upsamplers over a lattice of neighbour values.  Each builder gives (file bytes, expected pixels); the expectation is the
sequential model's pixel stage on the coefficients the file was written from (tests/jpeg_decode_model.py; the CPU tests hold
it against live Pillow), or a formula written out here.  Built once, shared, never changed."""
import numpy as np

import jpeg_decode_model as M
import jpeg_write as W

_cache = {}
ONES = np.ones(64, np.int64)
# The weights of the header's bound (a): W(d) = sum A_r A_c |d_rc| <= 65000
A = np.array([8192, 32501, 10703, 71869, 8192, 50643, 19570, 35521]) / 8192.0
BOUND = 65000.0
DENSE_SEED = 20261020


def shared(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def expected(width, height, comps, q, coefs):
    """The model's pixels of a file written from these (natural-order) tables and coefficients"""
    f = M.frame(width, height, comps, {t: [int(np.asarray(v).reshape(64)[M.ZIGZAG[i]]) for i in range(64)] for t, v in q.items()})
    return M.pixels(f, [np.asarray(c, np.int64)[..., M.ZIGZAG] for c in coefs])[2]


# ---- the IDCT ------------------------------------------------------------------------------------------------------------------
def samples(d):
    """Dequantised blocks (n, 64), natural order -> the model's descaled samples (n, 8, 8) in front of + 128 and the clamp"""
    return M.unclamped(np.asarray(d, np.int64).reshape(-1, 8, 8))


def inside_b(d):
    s = samples(d)
    return (s.min((1, 2)) >= -512) & (s.max((1, 2)) <= 511)


def largest_lone(k, sign, dc):
    """Per entry of the three arrays: the largest a for which a block of DC dc and coefficient k = sign * a (k = 0: dc + sign * a)
    keeps every sample in -512..511, read from the model's unclamped output by bisection — every a is checked to stay inside
    and a + 1 to leave"""
    k, sign, dc = (np.asarray(v, np.int64) for v in (k, sign, dc))
    rows = np.arange(k.size)

    def ok(a):
        d = np.zeros((k.size, 64), np.int64)
        d[:, 0] = dc
        d[rows, k] += sign * a
        return inside_b(d)
    lo, hi = np.zeros(k.size, np.int64), np.full(k.size, 8192, np.int64)  # ok(lo), not ok(hi)
    assert ok(lo).all() and not ok(hi).any()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        good = ok(mid)
        lo, hi = np.where(good, mid, lo), np.where(good, hi, mid)
    assert ok(lo).all() and not ok(lo + 1).any()
    return lo


def basis_blocks(q):
    """[(natural index, coefficient, DC)] of the sweep, QUANTISED by the flat table q: per position and sign the largest lone
    amplitude inside -512..511 (rounded down to a multiple of q, and to what baseline Huffman coding can hold: magnitude 1023)
    and half of it; then the same on DC = +-1016 (rounded to q), with the largest amplitude of that DC"""
    combos = [(k, sign, dc) for dc in (0, 1016 // q, -(1016 // q)) for k in range(0 if dc == 0 else 1, 64) for sign in (1, -1)]
    k, sign, dc = (np.array(v) for v in zip(*combos))
    top = np.minimum(largest_lone(k, sign, dc * q) // q, 1023)
    out = []
    for i, (kk, ss, dd) in enumerate(combos):
        out += [(kk, ss * int(top[i]), dd), (kk, ss * int(top[i] // 2), dd)]
    return out


def dense_blocks(count, seed, q):
    """`count` blocks with all 64 coefficients set, 0.6 .. 0.9 of the bound (a) and inside (b): seeded candidates are drawn until
    `count` satisfy both"""
    rng = np.random.default_rng(seed)
    out = []
    weights = (A[:, None] * A[None, :]).reshape(64)
    while len(out) < count:
        m = rng.integers(20, 120)
        d = rng.integers(1, m + 1, 64) * rng.choice([-1, 1], 64)
        d = (d * (rng.uniform(0.6, 0.9) * BOUND / (np.abs(d) * weights).sum())).astype(np.int64) // q
        d[d == 0] = 1
        d[0] = 0
        w = (np.abs(d * q) * weights).sum()
        if 0.6 * BOUND <= w <= 0.9 * BOUND and np.abs(d).max() <= 1023 and inside_b(d[None] * q)[0]:
            out.append(d)
    return out


def idct_sweep(q):
    """One gray image 33 blocks across: the basis blocks, then 200 dense ones.  q: the value of every entry of its 16-bit DQT"""
    def build():
        blocks = []
        for k, c, dc in basis_blocks(q):
            z = np.zeros(64, np.int64)
            z[0] = dc
            z[k] += c
            blocks.append(z)
        blocks += dense_blocks(200, DENSE_SEED, q)
        across = 33
        down = -(-len(blocks) // across)
        coefs = np.zeros((down * across, 64), np.int64)
        coefs[:len(blocks)] = blocks
        coefs = [coefs.reshape(down, across, 64)]
        width, height, table = across * 8 - 3, down * 8 - 5, {0: ONES * q}
        data = W.write(width, height, W.gray(), table, coefs, q16=(0,))
        return data, expected(width, height, W.gray(), table, coefs), len(blocks)
    return shared(("idct", q), build)


# ---- scaled quantisation tables ------------------------------------------------------------------------------------------------
def scale_dqt(data, factor):
    """Every 8-bit DQT of the file rewritten with 16-bit entries, times `factor`"""
    out, p = bytearray(data[:2]), 2
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        seg = data[p:p + 2 + n]
        if m == 0xDB:
            body, o = bytearray(), 4
            while o < len(seg):
                assert seg[o] >> 4 == 0
                body += bytes([0x10 | seg[o]]) + b"".join((v * factor).to_bytes(2, "big") for v in seg[o + 1:o + 65])
                o += 65
            seg = b"\xff\xdb" + (len(body) + 2).to_bytes(2, "big") + bytes(body)
        out += seg
        p += 2 + n
        if m == 0xDA:
            return bytes(out) + data[p:]


SCALED = ("gray_50x37_q80", "420_50x37_q80", "444_50x37_q95")


def scaled(name, factor):
    """(file, the model's pixels) of a committed case with its tables times `factor`"""
    import jpeg_decode_cases as JC

    def build():
        data = scale_dqt(JC.data(JC.by_name(name)), factor)
        return data, M.decode(data)[2]
    return shared(("scaled", name, factor), build)


# ---- colour conversion ---------------------------------------------------------------------------------------------------------
def jdcolor(y, cb, cr):
    """jdcolor.c's YCbCr -> RGB: 16-bit fixed point, FIX(x) = round(x * 65536), one half added once per sum"""
    y, cb, cr = (np.asarray(v, np.int32) for v in (y, cb, cr))  # (116130 * 127 is far inside 32 bits)
    r = y + ((91881 * (cr - 128) + 32768) >> 16)                          # FIX(1.40200)
    g = y + ((-22554 * (cb - 128) - 46802 * (cr - 128) + 32768) >> 16)    # FIX(0.34414), FIX(0.71414)
    b = y + ((116130 * (cb - 128) + 32768) >> 16)                         # FIX(1.77200)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


COLOUR_IMAGES = ("cbcr_y0", "cbcr_y128", "cbcr_y255", "ycr_cb128", "ycb_cr128")


def colour_values(name, rows=range(256)):
    """(Y, Cb, Cr) per block, block row = the first variable's values `rows`, block column = the second variable 0..255"""
    down, across = np.meshgrid(np.asarray(list(rows), np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    if name.startswith("cbcr_y"):
        return np.full(down.shape, int(name[6:])), down, across
    return (down, np.full(down.shape, 128), across) if name == "ycr_cb128" else (down, across, np.full(down.shape, 128))


def colour_image(name, rows=range(256)):
    """(file, per-block expectation (blocks down, 256, 3)): 4:4:4, q = 1, DC only: a DC of 8 (v - 128) is the flat sample v,
    since ((4 DC + 16) >> 5) + 128 = v.  All 256 block rows make the 2048 x 2048 image; fewer, a strip of it."""
    rows = list(rows)

    def build():
        ycc = colour_values(name, rows)
        coefs = []
        for v in ycc:
            z = np.zeros(v.shape + (64,), np.int64)
            z[..., 0] = 8 * (v - 128)
            coefs.append(z)
        data = W.write(2048, 8 * len(rows), W.colour("444"), {0: ONES, 1: ONES}, coefs)
        return data, jdcolor(*ycc)
    return shared(("colour", name, tuple(rows)), build)


# ---- upsamplers ----------------------------------------------------------------------------------------------------------------
LATTICE = [(a, b) for a in range(0, 256, 17) for b in range(0, 256, 17)] + [(0, 255), (255, 0), (1, 2), (254, 255)]
STRIPE_W, STRIPE_H = 34, 6  # chroma blocks: a stripe crosses a tile seam both ways and meets the halo


def upsampler_image(mode, trim, pairs=None):
    """(file, expected pixels): luma flat at 128, chroma DC only; stripe s of 6 chroma block rows alternates pair s's values — in
    columns for 4:2:2, in a checkerboard for 4:2:0 —, Cb with (a, b) and Cr with (b, a).  The image is `trim` (1 or 2) pixels
    short of its MCUs each way, so that the right and bottom edges replicate the last REAL sample.  The expectation: every
    chroma block is its flat value (colour_image says why, and the colour images test it), the real samples of those planes
    through the model's upsampler, then jdcolor() above — the model's own pixel stage gives the same and takes three times as long."""
    pairs = LATTICE if pairs is None else pairs

    def build():
        comps = W.colour(mode)
        v = comps[0]["v"]
        by, bx = np.mgrid[0:STRIPE_H * len(pairs), 0:STRIPE_W]
        a, b = (np.array([p[i] for p in pairs], np.int64)[by // STRIPE_H] for i in (0, 1))
        first = (bx % 2 == 0) if mode == "422" else ((bx + by) % 2 == 0)
        coefs = [np.zeros((by.shape[0] * v, STRIPE_W * 2, 64), np.int64)]
        width, height, up = 2 * 8 * STRIPE_W - trim, v * 8 * by.shape[0] - trim, []
        for value in (np.where(first, a, b), np.where(first, b, a)):
            z = np.zeros(by.shape + (64,), np.int64)
            z[..., 0] = 8 * (value - 128)
            coefs.append(z)
            real = np.repeat(np.repeat(value, 8, 0), 8, 1)[:-(-height // v), :-(-width // 2)]
            up.append((M._h2v1(real) if mode == "422" else M._h2v2(real))[:height, :width].astype(np.int32))
        return W.write(width, height, comps, {0: ONES, 1: ONES}, coefs), jdcolor(np.int32(128), *up)
    return shared(("up", mode, trim, tuple(pairs)), build)
