"""PNG encode of images of individual sizes and colour types on the device (`png.encode_images*`).  Throughout, file i is held
against the single-image entry's file (`encode_device`, with `options.quantization` its lossy twin) for image i, called
separately in the same process: byte for byte.  The shapes are the smallest at which the ragged filter form can go wrong; the
content is `synth.lcg_bytes` noise, so that a row read from the neighbouring image — as the row above, or through a wrong
offset — changes bytes, and `synth.scene` where a test needs matches."""
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

GRAY, GA, RGB, RGBA = 0, 1, 2, 3
# the six of the issue, interleaved so that the launch classes alternate
SIX = [(5, 3, GRAY), (7, 40, GA), (97, 53, RGB), (64, 65, RGBA), (1, 1, RGB), (130, 33, RGBA)]


def png():
    from pixo_amd import png as P
    return P


def cuda(px):
    import torch
    return torch.from_numpy(np.ascontiguousarray(px, dtype=np.uint8).reshape(-1).copy()).cuda()


def routes(clear=True):
    from pixo_amd import _lib
    return int(_lib.load().pixo_hip_debug_routes(1 if clear else 0))


def opts(preset=None, strategy=None, flags=0, quantization=None, w=0, h=0, ct=RGBA):
    from pixo_amd import ColorType
    P = png()
    b = P.PngOptions.builder(w, h).color_type(ColorType(ct))
    if preset is not None:
        b = b.preset(preset)
    if strategy is not None:
        b = b.filter_strategy(P.FilterStrategy(strategy))
    o = b.flags(flags).build()
    if quantization is not None:
        o.quantization = quantization
    return o


def for_image(o, w, h, ct):
    """the template with one image's width, height and colour type written into it"""
    from pixo_amd import ColorType
    import copy
    one = copy.copy(o)
    one.width, one.height, one.color_type = w, h, ColorType(ct)
    return one


def content(shapes, seed, scene=False):
    out = []
    for i, (w, h, ct) in enumerate(shapes):
        if scene:
            rgb = synth.scene(w, h, seed + i).reshape(h, w, 3)
            out.append(np.concatenate([rgb, 255 - rgb[:, :, :1] // 3], axis=2).reshape(-1) if ct == RGBA else rgb.reshape(-1))
        else:
            out.append(synth.lcg_bytes(w * h * (ct + 1), seed + i))
    return out


def lay_out(shapes, pixels, lead=0, gap=0, fill=0x11, align=1):
    """-> (block as a numpy array, records (width, height, ColorType, offset)): image i behind `lead` + the images in front,
    `gap` bytes of `fill` between two images, every offset rounded up to `align`"""
    from pixo_amd import ColorType
    records, at = [], lead
    for (w, h, ct), px in zip(shapes, pixels):
        at = -(-at // align) * align
        records.append((w, h, ColorType(ct), at))
        at += px.size + gap
    block = np.full(at + 16, fill, np.uint8)
    for (_, _, _, off), px in zip(records, pixels):
        block[off:off + px.size] = px
    return block, records


_SINGLES = {}


def singles(shapes, pixels, o, key=None):
    """the yardstick: one call of the single entry per image (kept per `key`: a reference is computed once)"""
    if key is not None and key in _SINGLES:
        return _SINGLES[key]
    got = [png().encode_device(cuda(px), for_image(o, w, h, ct)) for (w, h, ct), px in zip(shapes, pixels)]
    if key is not None:
        _SINGLES[key] = got
    return got


# ---- 1. colour types and strategies ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, 1], ids=["rayon", "no_rayon"])
@pytest.mark.parametrize("strategy", list(range(9)))
def test_colour_types_and_strategies(strategy, flags):
    P = png()
    pixels = content(SIX, 100)
    o = opts(strategy=strategy, flags=flags)
    want = singles(SIX, pixels, o)
    block, records = lay_out(SIX, pixels, align=16)
    plan = P.encode_images_plan(records, o)
    routes()
    got = P.encode_images_device(cuda(block), records, o)
    r = routes()
    for i in range(len(SIX)):
        assert got[i] == want[i], (i, SIX[i])
    assert r & P.ROUTE_PNG_IMAGES and not r & P.ROUTE_PNG_BATCH and not r & P.ROUTE_PNG_BATCH_FILTER and not r & P.ROUTE_SUB_BATCHES
    assert bool(r & P.ROUTE_PNG_IMAGES_FILTER) == any(plan["way_in"])
    if strategy != int(P.FilterStrategy.ADAPTIVE_FAST):
        assert all(plan["way_in"])
    elif flags:
        assert plan["way_in"] == [True, True, False, False, True, False]  # (areas of at most 4096 run Sub: nothing sequential about them)
    else:
        assert plan["way_in"] == [True, True, True, True, True, True]  # 97 x 53 and the others above the area rule are taller than 32


# ---- 2. row-length classes -------------------------------------------------------------------------------------------------

LONG = [4096, 4097, 8192, 8193, 12300]  # x 4 bytes: the last row of 256 threads' registers, the first of 512's, either side of 32 KiB, past the stage


@pytest.mark.parametrize("strategy", [6, 8], ids=["adaptive", "bigrams"])
def test_row_length_classes(strategy):
    P = png()
    shapes = []
    for w in LONG:
        shapes += [(w, 2, RGBA), (9, 9, RGB)]
    pixels = content(shapes, 200)
    o = opts(strategy=strategy)
    want = singles(shapes, pixels, o)
    block, records = lay_out(shapes, pixels, align=16)
    plan = P.encode_images_plan(records, o)
    assert all(plan["way_in"]) and plan["filter_launches"] == (5 if strategy == 6 else 4)  # RGBA: registers, 512 threads' registers, staged, direct (Bigrams: registers, staged, direct); RGB 9 x 9: Sub
    routes()
    got = P.encode_images_device(cuda(block), records, o)
    assert routes() & P.ROUTE_PNG_IMAGES_FILTER
    for i in range(len(shapes)):
        assert got[i] == want[i], (i, shapes[i])


# ---- 3. alignment ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lead", [0, 1, 7, 16])
def test_alignment_and_gaps(lead):
    P = png()
    shapes = SIX + [(64, 70, RGBA), (100, 50, GRAY)]  # (rows that are multiples of 4 bytes: aligned or not by their place alone)
    pixels = content(shapes, 300)
    o = opts(strategy=int(P.FilterStrategy.ADAPTIVE))
    want = singles(shapes, pixels, o, key="alignment")
    files = []
    for fill in (0xA5, 0x5A):
        block, records = lay_out(shapes, pixels, lead=lead, gap=5, fill=fill)
        files.append(P.encode_images_device(cuda(block), records, o))
    assert files[0] == files[1], "the bytes between the images changed a file"
    for i in range(len(shapes)):
        assert files[0][i] == want[i], (i, shapes[i], lead)
    # the images overlapping each other: the same image three times at the same place, and a second one inside the first
    block, records = lay_out(shapes[3:4], pixels[3:4], lead=lead)
    w, h, ct, at = records[0]
    inner = (64, 30, ct, at + 64 * 4 * 10)
    got = P.encode_images_device(cuda(block), [records[0], records[0], inner, records[0]], o)
    assert got[0] == got[1] == got[3] == want[3]
    assert got[2] == P.encode_device(cuda(pixels[3][64 * 4 * 10:64 * 4 * 40]), for_image(o, 64, 30, RGBA))


# ---- 4. mixed ways in --------------------------------------------------------------------------------------------------------

def test_sequential_and_batched_images_in_one_sub_batch():
    P = png()
    shapes = [(200, h, RGBA) for h in (1, 2, 32, 33, 64)] + [(300, 20, RGB)]
    pixels = content(shapes, 400, scene=False)
    o = opts(strategy=int(P.FilterStrategy.ADAPTIVE_FAST))
    block, records = lay_out(shapes, pixels, align=16)
    plan = P.encode_images_plan(records, o)
    assert plan["way_in"] == [True, True, False, True, True, False] and plan["sub_first"] == [0, 6]
    want = singles(shapes, pixels, o)
    routes()
    got = P.encode_images_device(cuda(block), records, o)
    r = routes()
    assert got == want
    assert r & P.ROUTE_PNG_IMAGES and r & P.ROUTE_PNG_IMAGES_FILTER


@pytest.mark.parametrize("preset", [1, 2])
def test_reductions_go_image_by_image(preset):
    P = png()
    shapes = [(97, 53, RGB), (64, 65, RGBA), (40, 30, GA), (33, 21, GRAY), (128, 96, RGBA)]
    pixels = content(shapes[:4], 500) + content(shapes[4:], 510, scene=True)
    pixels[1] = pixels[1].copy()
    pixels[1][3::4] = 255  # an opaque RGBA image: the colour type reduction has something to do
    o = opts(preset=preset)
    block, records = lay_out(shapes, pixels, lead=1, gap=3)
    assert P.encode_images_plan(records, o, alignment=0)["way_in"] == [False] * 5
    want = singles(shapes, pixels, o)
    routes()
    got = P.encode_images_device(cuda(block), records, o)
    r = routes()
    assert got == want
    assert r & P.ROUTE_PNG_IMAGES and not r & P.ROUTE_PNG_IMAGES_FILTER
    assert want[1][25] == 2, "the opaque RGBA image was not reduced to RGB"


def test_quantization_matches_the_lossy_single_entry():
    P = png()
    shapes = [(64, 64, RGBA)] * 4
    pixels = content(shapes, 600, scene=True)
    q = P.QuantizationOptions(P.QuantizationMode.FORCE, 64, True)
    for preset in (0, 1):
        o = opts(preset=preset, quantization=q)
        want = singles(shapes, pixels, o)
        assert all(f[25] == 3 for f in want), "the forced files are not indexed"
        block, records = lay_out(shapes, pixels, align=16)
        assert P.encode_images_device(cuda(block), records, o) == want


# ---- 5. the denser effort ----------------------------------------------------------------------------------------------------

def test_effort_high():
    P = png()
    shapes = [(200, 150, RGB), (64, 64, RGBA), (31, 17, GRAY)]
    pixels = content(shapes[:2], 700, scene=True) + content(shapes[2:], 702)
    o = opts(preset=0, flags=P.EFFORT_HIGH)
    want = singles(shapes, pixels, o)
    plain = singles(shapes, pixels, opts(preset=0))
    assert want[0] != plain[0], "the effort changed nothing on scene content"
    block, records = lay_out(shapes, pixels, align=16)
    assert P.encode_images_device(cuda(block), records, o) == want


# ---- 6. sub-batches ------------------------------------------------------------------------------------------------------------

def test_sub_batch_boundary_mid_batch():
    from pixo_amd import jpeg
    P = png()
    shapes = [(97, 53, RGB), (64, 65, RGBA), (7, 40, GA), (130, 33, RGBA), (5, 3, GRAY), (97, 53, RGB), (64, 65, RGBA)]
    full = [h * (w * (ct + 1) + 1) for w, h, ct in shapes]
    pixels = content(shapes, 800)
    o = opts(strategy=int(P.FilterStrategy.ADAPTIVE))
    want = singles(shapes, pixels, o)
    block, records = lay_out(shapes, pixels, align=16)
    d_block = cuda(block)
    limit = full[0] + full[1] + full[2] + 1  # three images, then the next three or four
    try:
        jpeg.debug_configure("png_batch_bytes=%d" % limit)
        plan = P.encode_images_plan(records, o)
        assert len(plan["sub_first"]) > 2 and plan["sub_first"][1] == 3
        routes()
        got = P.encode_images_device(d_block, records, o)
        r = routes()
    finally:
        jpeg.debug_configure(None)
    assert r & P.ROUTE_SUB_BATCHES and r & P.ROUTE_PNG_IMAGES_FILTER
    assert got == want
    routes()
    assert P.encode_images_device(d_block, records, o) == want and not routes() & P.ROUTE_SUB_BATCHES


def test_sub_batches_are_capped_by_chunks():
    P = png()
    n = 1100
    shapes = [(1 + i % 3, 1 + i % 2, i % 4) for i in range(n)]
    sizes = [w * h * (ct + 1) for w, h, ct in shapes]
    pixels = np.split(synth.lcg_bytes(sum(sizes), 900), np.cumsum(sizes)[:-1])  # (one stream of noise, cut into the images)
    o = opts(preset=0)
    block, records = lay_out(shapes, pixels)
    assert P.encode_images_plan(records, o)["sub_first"] == [0, 1024, n]
    d_block = cuda(block)
    routes()
    got = P.encode_images_device(d_block, records, o)
    assert routes() & P.ROUTE_SUB_BATCHES
    for i in list(range(0, n, 97)) + [1022, 1023, 1024, 1025, n - 1]:  # a sample, and both sides of the boundary
        w, h, ct = shapes[i]
        assert got[i] == P.encode_device(cuda(pixels[i]), for_image(o, w, h, ct)), i


# ---- 7. the chain: decode batch -> encode images -> decode ---------------------------------------------------------------------

CHAIN = ["gradient_128x96_c0_p1.png", "gradient_128x96_c1_p0.png", "gradient_128x96_c2_p0.png", "gradient_128x96_c3_p0.png",
         "flat_96x64_c3_p2.png", "grays_n16_97x53_c2_p1.png"]


def test_decode_batch_feeds_encode_images():
    from pixo_amd import decode
    P = png()
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_files")
    files = [open(os.path.join(here, name), "rb").read() for name in CHAIN]
    views = decode.decode_png_batch_device(files)
    assert len({int(ct) for _, ct in views}) >= 3, "the fixtures decode to fewer than three colour types"
    o = opts(preset=0)
    routes()
    again = P.encode_images_device(None, views, o)  # the views carry their block with them
    assert routes() & P.ROUTE_PNG_IMAGES
    info, total = decode.decode_png_batch_info(files)
    for (view, ct), file_bytes, (w, h, ict, _) in zip(views, again, info):
        image = decode.decode_png(file_bytes)
        assert (image.width, image.height, image.color_type) == (w, h, ict) == (view.shape[1], view.shape[0], ct)
        assert bytes(image.pixels) == view.cpu().numpy().tobytes()
        assert file_bytes == P.encode_device(view.contiguous(), for_image(o, w, h, int(ct)))
    # the same through the records and the block
    assert P.encode_images_device(views[0][0].data_ptr(), info, o) == again


# ---- 8. sinks --------------------------------------------------------------------------------------------------------------------

def test_into_arena_size_query_and_refusals():
    import torch
    from pixo_amd.error import BufferTooSmall, Error as PixoError
    P = png()
    pixels = content(SIX, 100)
    o = opts(strategy=int(P.FilterStrategy.ADAPTIVE))
    block, records = lay_out(SIX, pixels, lead=1, gap=2)
    d_block = cuda(block)
    want = P.encode_images_device(d_block, records, o)
    assert want == singles(SIX, pixels, o)
    n = len(SIX)
    offsets, lens = P.encode_images_device_into(None, d_block, records, o)  # the size query
    assert lens == [len(f) for f in want] and offsets == [sum(lens[:i]) for i in range(n)]
    total = offsets[-1] + lens[-1]
    for base in (torch.full((total + 8,), 0xEE, dtype=torch.uint8), torch.full((total + 8,), 0xEE, dtype=torch.uint8).pin_memory(),
                 np.full(total + 8, 0xEE, np.uint8)):
        for shift in (0, 1):
            arena = base[shift:]
            assert P.encode_images_device_into(arena, d_block, records, o) == (offsets, lens)
            flat = arena.numpy() if hasattr(arena, "numpy") else arena
            assert [flat[a:a + k].tobytes() for a, k in zip(offsets, lens)] == want
            assert bytes(flat[total:]) == b"\xEE" * (flat.size - total)
    short = np.full(total - 1, 0xEE, np.uint8)
    with pytest.raises(BufferTooSmall) as e:
        P.encode_images_device_into(short, d_block, records, o)
    assert str(e.value) == "output buffer too small: need %d bytes" % total
    assert (e.value.offsets, e.value.lens, e.value.needed) == (offsets, lens, total)
    assert bytes(short) == b"\xEE" * (total - 1), "the refused call wrote into the arena"
    with pytest.raises(PixoError):  # a device arena is refused
        P.encode_images_device_into(torch.zeros(total, dtype=torch.uint8, device="cuda"), d_block, records, o)
    with pytest.raises(ValueError):  # the wrapper checks a tensor's size against the records
        P.encode_images_device(d_block[:100], records, o)
    assert P.encode_images_device(d_block, records, o) == want  # the next call on the same thread
    # the host entry: the same block in host memory, twice
    assert P.encode_images(block, records, o) == want
    assert P.encode_images(block.tobytes(), records, o) == want
