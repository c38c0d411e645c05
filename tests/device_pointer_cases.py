"""Caller pointers of every alignment for the PNG, zlib and decode device entries: a device buffer with canary bytes on both
sides of a view that starts `offset` bytes past an aligned address, the fixed (input, output) offset pairs, and the case
tables of tests/test_gpu_device_pointers.py, each case with the path it claims to reach.  The claims are pinned with the
models alone by tests/test_device_pointer_cases_cpu.py.  Test harness only; torch is imported when a buffer is made."""
import zlib

import numpy as np

import png_decode_cases as PC
import png_file_cases as FC
import png_quantize_cases as QC
import synth

PAD, FILL = 64, 0xA5

# (input offset, output offset): 1-3 flip every `% 4` predicate, 4 and 8 keep `% 4` and flip `% 16`, (16, 16) is a base
# other than the allocation's own that keeps every fast path
IN_OUT = [(1, 3), (2, 1), (3, 2), (4, 8), (8, 4), (0, 1), (1, 0), (16, 16)]
OUT_FOR = {1: 3, 2: 1, 3: 2, 4: 8, 8: 4, 16: 16}  # the first pair of IN_OUT with that input offset


def _bytes(data):
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, np.uint8)
    return np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)


def at_offset(host_bytes_or_size, offset, pad=PAD, fill=FILL):
    """-> (whole, view): a device uint8 tensor filled with `fill`, and its slice of n bytes that starts `offset` bytes past
    the `pad` canary bytes in front (pad is a multiple of 64: the view's address is `offset` modulo 64).  Given data, the
    view holds it; given a size, the view is canary too.  `pad` bytes follow the view."""
    import torch
    assert pad % 64 == 0 and pad > 0 and offset >= 0
    data = None if isinstance(host_bytes_or_size, (int, np.integer)) else _bytes(host_bytes_or_size)
    n = int(host_bytes_or_size) if data is None else data.size
    host = np.full(pad + offset + n + pad, fill, np.uint8)
    if data is not None:
        host[pad + offset:pad + offset + n] = data
    whole = torch.from_numpy(host).to("cuda:0")
    view = whole[pad + offset:pad + offset + n]
    torch.cuda.synchronize()
    assert view.data_ptr() % 64 == offset % 64, "the allocation itself is not 64-byte aligned: the offsets would not mean what they say"
    return whole, view


def untouched(whole, offset, n, pad=PAD, fill=FILL):
    """Every byte of `whole` outside the view at_offset(.., offset) of n bytes is still `fill`."""
    got = whole.cpu().numpy()
    assert got.size == pad + offset + n + pad
    return bool((got[:pad + offset] == fill).all() and (got[pad + offset + n:] == fill).all())


# ---- A. row filters ----------------------------------------------------------------------------------------------------------
def filter_content(w, h, bpp, seed):
    """The two contents of test_every_strategy_and_pixel_size_against_the_oracle in one image: noise rows above, a `cumsum`
    ramp below, so that the adaptive strategies choose different filters in the two halves"""
    px = synth.lcg_bytes(w * h * bpp, seed + bpp)
    half = (h // 2) * w * bpp
    px[half:] = (np.cumsum(px[half:].astype(np.int64) % 5) % 256).astype(np.uint8)
    return px


ALL_PAIRS = list(IN_OUT)
FILTER_CASES = [
    dict(name="A1_128x40_bpp%d" % bpp, w=128, h=40, bpp=bpp, strategies=list(range(9)), pairs=ALL_PAIRS, row_mod4=0, stateful=False,
         path="row_bytes % 4 == 0: the base alone decides FAST") for bpp in (1, 2, 3, 4, 6, 8)
] + [
    dict(name="A2_127x40_bpp%d" % bpp, w=127, h=40, bpp=bpp, strategies=list(range(9)), pairs=ALL_PAIRS, row_mod4=mod, stateful=False,
         path="row_bytes % 4 != 0 and the base % 4 != 0 at once") for bpp, mod in ((1, 3), (3, 1))
] + [
    dict(name="A3_%dx34_bpp4" % w, w=w, h=34, bpp=4, strategies=[5, 6, 7, 8], pairs=[(1, 3), (2, 1)], row_mod4=0, stateful=False, path=path)
    for w, path in ((4100, "just past the 16 KiB register form"), (8200, "just past the 32 KiB register form"),
                    (12600, "50,400-byte rows: past the 48 KiB LDS stage, direct stores"))
] + [
    dict(name="A4_300x32_bpp4", w=300, h=32, bpp=4, strategies=[7], pairs=[(1, 3), (3, 2)], row_mod4=0, stateful=True,
         path="h = 32: the two-launch sequential AdaptiveFast"),
]
ADAPTIVE = (5, 6, 7, 8)

# ---- B. reductions -----------------------------------------------------------------------------------------------------------
REDUCE_WIDTHS, REDUCE_HEIGHT = (72, 71, 70, 73), 67  # npix % 4 = 0, 1, 2, 3; more than 4096 pixels
REDUCE_IN_OFFSETS = (1, 2, 3, 4, 8, 16)
# options: preset 0 (no reduction: the filter reads the caller's pointer), preset 1, and preset 1 without reduce_palette
# (a gray-valued image has at most 256 colours: with the palette switch on it becomes indexed before it can become gray)
# class -> (colour types, {options: claimed outcome}); outcomes: "unchanged", ("indexed", depth), "gray", "gray_alpha", "rgb",
# "zero_alpha" (layout unchanged, colour under alpha 0 cleared)
REDUCE_CLASSES = {
    "pal5": ((2, 3), {"p0": "unchanged", "p1": ("indexed", 4)}),            # co-occurrence counters in LDS
    "pal200": ((2, 3), {"p0": "unchanged", "p1": ("indexed", 8)}),          # ... in global memory
    "gray": ((2, 3), {"p0": "unchanged", "p1": ("indexed", 8), "p1_nopal": "gray"}),
    "gray_some_alpha": ((3,), {"p0": "unchanged", "p1": "gray_alpha"}),    # more than 256 (gray, alpha) pairs
    "opaque": ((3,), {"p0": "unchanged", "p1": "rgb"}),
    "alpha0": ((1, 3), {"p0": "unchanged", "p1": "zero_alpha"}),
    "noise": ((1, 2, 3), {"p0": "unchanged", "p1": "unchanged"}),           # nothing reduces: the filter reads the pointer itself
}
REDUCE_CASES = [dict(name="%s_c%d_%dx%d" % (cls, ct, w, REDUCE_HEIGHT), cls=cls, ct=ct, w=w, h=REDUCE_HEIGHT, outcomes=out)
                for cls, (cts, out) in REDUCE_CLASSES.items() for ct in cts for w in REDUCE_WIDTHS]
SPP = {0: 1, 1: 2, 2: 3, 3: 4}


def reduce_input(c):
    w, h, spp, cls = c["w"], c["h"], SPP[c["ct"]], c["cls"]
    rng = np.random.RandomState(w * 7 + c["ct"] * 1000 + len(cls))
    if cls in ("pal5", "pal200"):
        n = 5 if cls == "pal5" else 200
        cols = rng.randint(0, 256, (n, spp)).astype(np.uint8)
        cols[:, 1] |= 1  # (never gray)
        cols[:, 0] &= 0xFE
        img = cols[rng.randint(0, n, (h, w))]
    else:
        img = rng.randint(0, 256, (h, w, spp)).astype(np.uint8)
        if cls in ("gray", "gray_some_alpha"):
            img[:, :, 1] = img[:, :, 0]
            img[:, :, 2] = img[:, :, 0]
        if spp in (2, 4):
            a = img[:, :, spp - 1]
            if cls in ("gray", "opaque"):
                a[:] = 255
            else:
                a[a == 0] = 1  # "noise", "gray_some_alpha": some alpha, never 0
                if cls == "alpha0":
                    a[rng.rand(h, w) < 0.2] = 0
    return np.ascontiguousarray(img).reshape(-1)


def reduce_model_options(key):
    import png_reduce_model as M
    o = M.Opts.preset(0 if key == "p0" else 1, flags=M.NO_RAYON)
    if key == "p1_nopal":
        o.reduce_palette = False
    return o


def reduce_options(c, key):
    from pixo_amd import ColorType, png
    b = png.PngOptions.builder(c["w"], c["h"]).color_type(ColorType(c["ct"])).preset(0 if key == "p0" else 1).flags(png.NO_RAYON)
    if key == "p1_nopal":
        b = b.reduce_palette(False)
    return b.build()


# ---- C. quantisation (Force) ---------------------------------------------------------------------------------------------------
# (w, h, colour type, n colours, seed, max_colors, dithering, early_out, dither form: "chained" / "banded" / None)
QUANT_CASES = [dict(c=QC.force_case(w, h, ct, n, seed), max_colors=mc, dithering=d, early_out=eo, form=form, path=path)
               for (w, h, ct, n, seed, mc, d, eo, form, path) in [
    (67, 129, 3, 1000, 8, 255, True, False, "chained", "RGBA, RawPixel<false> at spp 4 in the chained launch of 3 bands"),
    (131, 40, 3, 1000, 31, 256, True, False, "banded", "RGBA, RawPixel<false> at spp 4 in the one-band launch"),
    (130, 65, 3, 1000, 32, 256, False, False, None, "RGBA, pngq_map_kernel<false> at spp 4 through the LUT"),
    (130, 65, 3, 200, 33, 256, True, True, None, "RGBA, early out: pngq_map_kernel<false> at spp 4 without the LUT"),
    (67, 129, 2, 1000, 34, 255, True, False, "chained", "RGB, chained"),
    (131, 40, 2, 1000, 35, 256, True, False, "banded", "RGB, one band"),
    (130, 65, 2, 1000, 7, 256, False, False, None, "RGB, map through the LUT"),
    (130, 65, 2, 200, 36, 256, True, True, None, "RGB, early out"),
]]
QUANT_IN_OFFSETS = (1, 2, 3, 4)  # 1-3 flip ALIGNED4; 4 keeps it at a base that is not 16-byte aligned

# ---- D. zlib -------------------------------------------------------------------------------------------------------------------
ZLIB_LENGTHS = (1, 3, 65535, 65536, 2 * 65535 + 7)
ZLIB_MIXED_LEN, ZLIB_MIXED_ROW = 200000, 4 * 100 + 1


def zlib_cases():
    """(name, data, bpp, row, shrinks): noise of the listed lengths, and one input whose 20,000-byte stretches alternate
    between a smooth ramp and noise, so that compressed and stored blocks alternate"""
    out = [("noise_%d" % n, np.random.RandomState(n).randint(0, 256, n).astype(np.uint8).tobytes(), 0, 0, False) for n in ZLIB_LENGTHS]
    rng = np.random.RandomState(77)
    mixed = rng.randint(0, 256, ZLIB_MIXED_LEN).astype(np.uint8)
    for k, at in enumerate(range(0, ZLIB_MIXED_LEN, 20000)):
        if k % 2 == 0:
            mixed[at:at + 20000] = (np.cumsum(mixed[at:at + 20000].astype(np.int64) % 3) % 256).astype(np.uint8)
    return out + [("mixed_%d" % ZLIB_MIXED_LEN, mixed.tobytes(), 4, ZLIB_MIXED_ROW, True)]


def host_zlib_shrinks(data):
    return len(zlib.compress(data, 6)) < len(data)


# ---- E. decode -----------------------------------------------------------------------------------------------------------------
DECODE_OUT_OFFSETS = (0, 1, 2, 3, 4, 8, 16)
_ALPHA = bytes([0, 128])  # a tRNS with values other than 255: four output bytes a pixel


def _d(name, w, h, ct, depth, out_bpp, seed, path, trns=None, plte=None):
    row_out = w * out_bpp
    return dict(name=name, w=w, h=h, ct=ct, depth=depth, out_bpp=out_bpp, row_out_mod16=row_out % 16, total_mod4=row_out * h % 4,
                path=path, file=PC.make(w, h, ct, depth, seed=seed, trns=trns, plte_entries=plte))


DECODE_CASES = [
    _d("gray8_16x9", 16, 9, PC.GRAY, 8, 1, 101, "copy16 at a 16-byte base, the bytes kernel elsewhere"),
    _d("rgba8_4x9", 4, 9, PC.RGBA, 8, 4, 102, "copy16 at a 16-byte base, the bytes kernel elsewhere"),
    _d("rgb8_32x5", 32, 5, PC.RGB, 8, 3, 103, "copy16 at a 16-byte base, the bytes kernel elsewhere"),
    _d("rgb8_5x9", 5, 9, PC.RGB, 8, 3, 104, "bytes kernel, 135 bytes: a 3-byte tail"),
    _d("rgba16_8x9", 8, 9, PC.RGBA, 16, 4, 105, "bytes kernel, high-byte form"),
    _d("gray16_7x5", 7, 5, PC.GRAY, 16, 1, 106, "bytes kernel, high-byte form, 35 bytes"),
] + [
    _d("gray%d_13x9" % d, 13, 9, PC.GRAY, d, 1, 110 + d, "samples kernel, one output byte a pixel") for d in (1, 2, 4)
] + [
    _d("pal%d_%s_13x9" % (d, "trns" if t else "opaque"), 13, 9, PC.INDEXED, d, 4 if t else 3, 120 + d, "samples kernel, %s" % (
        "four bytes a pixel: dword or byte stores" if t else "three bytes a pixel: byte stores"), trns=t)
    for d in (1, 2, 4, 8) for t in (_ALPHA, None)
]

# ---- F. lossless whole files ---------------------------------------------------------------------------------------------------
FILE_IN_OFFSETS = (1, 2, 3, 8)


def file_cases():
    """Per colour type the smallest of png_file_cases.CASES (the first of its size in the file's order), and the same image
    under preset 1, whose reductions read the caller's pointer before the filters do"""
    out = []
    for ct in (0, 1, 2, 3):
        of_type = [c for c in FC.CASES if c["color_type"] == ct]
        smallest = min(of_type, key=lambda c: c["w"] * c["h"])
        out.append(smallest)
        out += [c for c in of_type if (c["gen"], c["w"], c["h"], c["seed"]) == (smallest["gen"], smallest["w"], smallest["h"], smallest["seed"])
                and c["preset"] == 1 and c is not smallest]
    return out
