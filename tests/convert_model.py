"""TEST HARNESS: the colour conversions restated in numpy, from their formulas (include/pixo_hip.h): GrayAlpha -> Gray takes
byte 0 of every pixel, Rgba -> Rgb bytes 0..2, Rgb / Rgba -> Gray is (77 r + 150 g + 29 b + 128) >> 8 with the alpha
ignored, equal types copy.  Colour types: 0 Gray, 1 GrayAlpha, 2 Rgb, 3 Rgba."""
import numpy as np

GRAY, GRAY_ALPHA, RGB, RGBA = 0, 1, 2, 3
OPAQUE, TO_GRAY = 0, 1
K_COPY, K_GA_G, K_RGBA_RGB, K_RGB_G, K_RGBA_G = range(5)
PAIRS = {K_GA_G: (GRAY_ALPHA, GRAY), K_RGBA_RGB: (RGBA, RGB), K_RGB_G: (RGB, GRAY), K_RGBA_G: (RGBA, GRAY)}


def bpp(ct):
    return ct + 1


def kind_of(src_ct, dst_ct):
    """The kind of a pair, None for a pair that does not exist"""
    if src_ct == dst_ct:
        return K_COPY
    for k, pair in PAIRS.items():
        if pair == (src_ct, dst_ct):
            return k
    return None


def target_type(target, src_ct):
    if target == TO_GRAY:
        return GRAY
    return {GRAY: GRAY, GRAY_ALPHA: GRAY, RGB: RGB, RGBA: RGB}[src_ct]


def luma(r, g, b):
    return (77 * r.astype(np.uint32) + 150 * g.astype(np.uint32) + 29 * b.astype(np.uint32) + 128) >> 8


def convert(px, src_ct, dst_ct) -> np.ndarray:
    """Flat uint8 pixels of src_ct -> flat uint8 pixels of dst_ct"""
    px = np.asarray(px, np.uint8).reshape(-1, bpp(src_ct))
    k = kind_of(src_ct, dst_ct)
    if k is None:
        raise ValueError("no such conversion: %d -> %d" % (src_ct, dst_ct))
    if k == K_COPY:
        return px.reshape(-1).copy()
    if k == K_GA_G:
        return px[:, 0].copy()
    if k == K_RGBA_RGB:
        return px[:, :3].reshape(-1).copy()
    return luma(px[:, 0], px[:, 1], px[:, 2]).astype(np.uint8)
