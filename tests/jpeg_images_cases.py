"""Shapes by group count for the JPEG images entry (`jpeg.encode_images*`), and what tests/test_jpeg_images_placement_cpu.py,
tests/test_gpu_jpeg_images.py and the child of tests/test_gpu_parity.py that forces the look-back fallback share: the long list,
its content, its layout in one block and its expectation.

A coding pass works in groups of 192 blocks of 64 coefficients: 32 MCUs of 6 blocks at 4:2:0, 64 units of 3 blocks at 4:4:4,
192 blocks of a gray image.  The two-level look-back (jpeg_scan_dev.h look_back_blocks) keeps one sum per 64 groups of a
segment: only a segment of at least 64 groups writes one, only one of at least 65 reads one, and a pass of at least 256 groups
keeps them in 16 copies.  SHAPES names sizes by the groups they have; nothing here is trusted by a test — each asserts the
counts from `jpeg.encode_images_plan`."""
import numpy as np

import synth

GRAY, RGB = 0, 2
GROUP = 192
CLASSES = ("444", "420", "gray")  # a colour class of a coding pass: RGB at the template's subsampling, or gray

# class -> groups -> (width, height), every last group full (the 1-group image aside: 25 or 9 units)
SHAPES = {
    "444": {1: (40, 40), 63: (504, 512), 64: (512, 512), 65: (520, 512), 128: (1024, 512), 129: (1032, 512)},
    "420": {1: (40, 40), 63: (512, 1008), 64: (512, 1024), 65: (512, 1040), 128: (1024, 1024), 129: (512, 2064)},
    "gray": {1: (40, 40), 63: (768, 1008), 64: (768, 1024), 65: (768, 1040), 128: (1536, 1024), 129: (768, 2064)},
}


def klass(ct, ss):
    return "gray" if ct == GRAY else ("420" if ss == 1 else "444")


def blocks(w, h, cls):
    unit = 16 if cls == "420" else 8
    units = -(-w // unit) * -(-h // unit)
    return units * {"444": 3, "420": 6, "gray": 1}[cls]


def groups(w, h, cls):
    return -(-blocks(w, h, cls) // GROUP)


def plan_groups(jpeg, records, o):
    """the groups of every record, from the plan entry's `first_group` alone: two one-group records, one per colour class, are
    appended so that the last image of a class has a successor"""
    from pixo_amd import ColorType
    p = jpeg.encode_images_plan(list(records) + [(8, 8, ColorType.Gray, 0), (8, 8, ColorType.Rgb, 0)], o)
    assert all(p["way_in"]) and len(p["sub_first"]) == 2, p["sub_first"]
    first, out = p["first_group"], []
    cts = [int(r[2]) for r in records] + [GRAY, RGB]
    for i in range(len(records)):
        out.append(next(first[j] for j in range(i + 1, len(cts)) if cts[j] == cts[i]) - first[i])
    return out


# ---- the long list -------------------------------------------------------------------------------------------------------------
# Per colour class: a one-group image first (the floors behind it are no multiples of 64), then segments of 65, 64, 129, 1 and 63
# groups, then the 64-group size one pixel larger each way (partial edge blocks, a last group of 1 unit / 1 MCU / 33 blocks).
# Content: noise; the 64-group RGB image and the 63-group gray image flat (equal aggregates, DC differences of zero behind the
# segment's first block); the second one-group RGB image a scene.  The gray and the RGB list interleaved.
_RGB = [(1, "n"), (65, "n"), (64, "255"), (129, "n"), (1, "scene"), (63, "n"), ("64+", "n")]
_GRAY = [(1, "n"), (65, "n"), (64, "n"), (129, "n"), (1, "n"), (63, "0"), ("64+", "n")]


def _shape(cls, key):
    if key == "64+":
        w, h = SHAPES[cls][64]
        return w + 1, h + 1
    return SHAPES[cls][key]


def long_list(ss):
    """-> (shapes (width, height, colour, content), the groups each is meant to have)"""
    rgb = klass(RGB, ss)
    shapes, claimed = [], []
    for (kr, cr), (kg, cg) in zip(_RGB, _GRAY):
        for cls, ct, key, what in ((rgb, RGB, kr, cr), ("gray", GRAY, kg, cg)):
            w, h = _shape(cls, key)
            shapes.append((w, h, ct, what))
            claimed.append(groups(w, h, cls) if key == "64+" else key)
    return shapes, claimed


ORDERS = ("list", "reversed", "tight")


def order(n, which):
    """the indices of an n-image long list in order `which`; tight: the 65-group image of either class in front (first group 0,
    65 groups: its two words of block sums end where the next segment's begin)"""
    idx = list(range(n))
    if which == "reversed":
        return idx[::-1]
    if which == "tight":
        return [2, 3, 0, 1] + idx[4:]
    return idx


def make_pixels(shapes, seed):
    out = []
    for i, (w, h, ct, what) in enumerate(shapes):
        n = w * h * (ct + 1)
        if what == "n":
            out.append(synth.lcg_bytes(n, seed + i))
        elif what == "scene":
            out.append(synth.scene(w, h, seed + i).reshape(-1))
        else:
            out.append(np.full(n, int(what), np.uint8))
    return out


def lay_out(shapes, pixels, idx=None, lead=0, gap=0, fill=0x11, align=1):
    """-> (block, records (width, height, ColorType, offset)) of the images idx (all, in order, when None): image after image
    behind `lead` bytes, `gap` bytes of `fill` between two, every offset rounded up to `align`"""
    from pixo_amd import ColorType
    idx = list(range(len(shapes))) if idx is None else idx
    records, at = [], lead
    for i in idx:
        w, h, ct, _ = shapes[i]
        at = -(-at // align) * align
        records.append((w, h, ColorType(ct), at))
        at += pixels[i].size + gap
    block = np.full(at + 16, fill, np.uint8)
    for i, (_, _, _, off) in zip(idx, records):
        block[off:off + pixels[i].size] = pixels[i]
    return block, records


def oracle_files(O, shapes, pixels, q, ss):
    return [O.encode(px, O.make_options(w, h, ct, q, ss)) for (w, h, ct, _), px in zip(shapes, pixels)]


def template(jpeg, ss, q):
    from pixo_amd import ColorType
    return jpeg.JpegOptions.builder(0, 0).color_type(ColorType.Rgb).quality(q).subsampling(jpeg.Subsampling(ss)).build()


# ---- the bounded waits giving up (run by the child of test_gpu_parity that starts under spin_budget=0) ------------------------

def give_up_of_the_images_entry():
    """With a budget of zero polls a group that has to wait for another raises the abort flag: code_pass returns
    kRetryMultipass, the sub-batch goes the single way (sink.at put back), FALLBACK is noted and the counter rises.  The long
    list at 4:2:0 into blocks and into a pinned arena, then in at least three sub-batches; every file, offset and length is
    the oracle's; JPEG_IMAGES is not noted, since no sub-batch's files came from the ragged launches.  Then the default
    budget: the same call notes no fallback.  Returns the fallbacks counted."""
    import torch
    import oracle_lib as O
    from pixo_amd import jpeg
    ss, q = 1, 80
    shapes, _ = long_list(ss)
    pixels = make_pixels(shapes, 700)
    want = oracle_files(O, shapes, pixels, q, ss)
    lens = [len(f) for f in want]
    offsets = [sum(lens[:i]) for i in range(len(lens))]
    o = template(jpeg, ss, q)
    block, records = lay_out(shapes, pixels, lead=1, gap=3)
    d_block = torch.from_numpy(block).cuda()
    n0 = jpeg.lookback_fallbacks()
    counted = []
    for switches in ("spin_budget=0", "spin_budget=0,jpeg_images_blocks=40000"):
        jpeg.debug_configure(switches)
        subs = len(jpeg.encode_images_plan(records, o)["sub_first"]) - 1
        assert subs == 1 if "blocks" not in switches else subs >= 3, subs
        before = jpeg.lookback_fallbacks()
        jpeg.debug_routes()
        got = jpeg.encode_images_device(d_block, records, o)
        r = jpeg.debug_routes()
        rose = jpeg.lookback_fallbacks() - before
        assert got == want, [i for i in range(len(want)) if got[i] != want[i]]
        assert r & jpeg.ROUTE_FALLBACK and not r & jpeg.ROUTE_JPEG_IMAGES and not r & jpeg.ROUTE_JPEG_IMAGES_DIRECT, hex(r)
        assert bool(r & jpeg.ROUTE_SUB_BATCHES) == (subs > 1)
        assert rose >= subs, (rose, subs)  # (every sub-batch holds a segment of 63 groups or more)
        arena = torch.full((sum(lens) + 5,), 0xEE, dtype=torch.uint8).pin_memory()
        jpeg.debug_routes()
        assert jpeg.encode_images_device_into(arena[:sum(lens)], d_block, records, o) == (offsets, lens)
        r = jpeg.debug_routes()
        assert r & jpeg.ROUTE_FALLBACK and not r & jpeg.ROUTE_JPEG_IMAGES, hex(r)
        flat = arena.numpy()
        assert [flat[a:a + k].tobytes() for a, k in zip(offsets, lens)] == want
        assert (flat[sum(lens):] == 0xEE).all()
        counted.append(jpeg.lookback_fallbacks() - before)
    jpeg.debug_configure("")  # the default budget, whatever the environment says
    try:
        before = jpeg.lookback_fallbacks()
        jpeg.debug_routes()
        got = jpeg.encode_images_device(d_block, records, o)
        r = jpeg.debug_routes()
        assert got == want
        assert r & jpeg.ROUTE_JPEG_IMAGES and not r & jpeg.ROUTE_FALLBACK and jpeg.lookback_fallbacks() == before, hex(r)
    finally:
        jpeg.debug_configure(None)  # back to the environment's switches
    assert jpeg.lookback_fallbacks() > n0
    return counted
