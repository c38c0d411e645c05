"""JPEG encode of images of individual sizes on the device (`jpeg.encode_images*`).  Throughout, file i is held against the
single-image entry's file (`jpeg.encode_device` with the template at image i's width, height and colour type) for image i,
uploaded alone: byte for byte.  For the basic set at preset 0 it is also held against tests/oracle_lib directly.  The shapes
are the smallest at which the ragged forms can go wrong; the content is `synth.lcg_bytes` noise, so that a wrong offset or a
neighbour's row changes bytes and 0xFF stuffing occurs, flat images for the DC predictors, and one `synth.scene`.
From section 9 on (segments of 63 to 4097 groups, the packed coefficient forms, files of 1 MB, the stuffing pass's retries,
call histories) the expectation is the oracle's file, and the single entry's file is held against it in the same test; the
bounded waits giving up are forced in the child process of test_gpu_parity (no test of this process may fall back)."""
import copy
import io

import numpy as np
import pytest

import jpeg_images_cases as K
import oracle_lib as O
import synth

pytestmark = pytest.mark.gpu

GRAY, RGB = 0, 2
# (width, height, colour, content): the issue's table, classes alternating; a flat 0 image directly in front of a flat 255
# image of the same size in both colour classes (a DC predictor leaking across a segment boundary changes bytes); one scene
BASIC = [(1, 1, RGB, "n"), (7, 9, GRAY, "n"), (16, 16, RGB, "n"), (512, 16, RGB, "n"), (520, 8, RGB, "n"), (513, 17, RGB, "n"),
         (1537, 9, GRAY, "n"), (97, 53, RGB, "n"), (8, 8, GRAY, "0"), (8, 8, GRAY, "255"), (24, 24, RGB, "0"), (24, 24, RGB, "255"),
         (64, 48, RGB, "scene")]


def J():
    from pixo_amd import jpeg
    return jpeg


def cuda(px):
    import torch
    return torch.from_numpy(np.ascontiguousarray(px, dtype=np.uint8).reshape(-1).copy()).cuda()


def opts(ss=1, q=80, preset=None):
    from pixo_amd import ColorType
    j = J()
    b = j.JpegOptions.builder(0, 0).color_type(ColorType.Rgb).quality(q)
    if preset is not None:
        return b.preset(preset).build()
    return b.subsampling(j.Subsampling(ss)).build()


def for_image(o, w, h, ct):
    from pixo_amd import ColorType
    one = copy.copy(o)
    one.width, one.height, one.color_type = w, h, ColorType(ct)
    return one


def content(shapes, seed):
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


def lay_out(shapes, pixels, lead=0, gap=0, fill=0x11, align=1):
    """-> (block, records (width, height, ColorType, offset)): image i behind `lead` + the images in front, `gap` bytes of
    `fill` between two images, every offset rounded up to `align`"""
    from pixo_amd import ColorType
    records, at = [], lead
    for (w, h, ct, _), px in zip(shapes, pixels):
        at = -(-at // align) * align
        records.append((w, h, ColorType(ct), at))
        at += px.size + gap
    block = np.full(at + 16, fill, np.uint8)
    for (_, _, _, off), px in zip(records, pixels):
        block[off:off + px.size] = px
    return block, records


_SINGLES = {}


def singles(shapes, pixels, o, key=None):
    """the yardstick: one call of the single entry per image, each uploaded alone (kept per `key`)"""
    if key is not None and key in _SINGLES:
        return _SINGLES[key]
    got = [J().encode_device(cuda(px), for_image(o, w, h, ct)) for (w, h, ct, _), px in zip(shapes, pixels)]
    if key is not None:
        _SINGLES[key] = got
    return got


def basic(ss, q=80):
    pixels = content(BASIC, 100)
    o = opts(ss, q)
    return pixels, o, singles(BASIC, pixels, o, key=("basic", ss, q))


# ---- 1. the basic set, routes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ss", [1, 0], ids=["420", "444"])
def test_basic_set_against_single_entry_and_oracle(ss):
    j = J()
    pixels, o, want = basic(ss)
    block, records = lay_out(BASIC, pixels, align=16)
    d_block = cuda(block)
    plan = j.encode_images_plan(records, o, alignment=d_block.data_ptr() % 16)
    assert all(plan["way_in"]) and plan["sub_first"] == [0, len(BASIC)] and plan["entropy_passes"] == 2
    j.debug_routes()
    got = j.encode_images_device(d_block, records, o)
    r = j.debug_routes()
    for i, (w, h, ct, _) in enumerate(BASIC):
        assert got[i] == want[i], (i, BASIC[i])
        assert got[i] == O.encode(pixels[i], O.make_options(w, h, ct, 80, ss)), (i, BASIC[i], "oracle")
    assert r & j.ROUTE_JPEG_IMAGES and r & j.ROUTE_TWO_KERNEL and r & j.ROUTE_SEGMENTED_TUPLE
    assert not r & j.ROUTE_BATCH_FUSED and not r & j.ROUTE_SUB_BATCHES and not r & j.ROUTE_FALLBACK
    assert j.lookback_fallbacks() == 0


@pytest.mark.parametrize("preset", [1, 2])
def test_presets_with_tables_or_scans_of_their_own_go_the_single_way(preset):
    j = J()
    shapes = [BASIC[i] for i in (0, 1, 2, 7, 8, 9, 12)]
    pixels = content(shapes, 200)
    o = opts(preset=preset)
    want = singles(shapes, pixels, o)
    block, records = lay_out(shapes, pixels, lead=1, gap=3)
    plan = j.encode_images_plan(records, o)
    assert plan["way_in"] == [False] * len(shapes) and plan["coef_launches"] == 0 and plan["entropy_passes"] == 0
    j.debug_routes()
    got = j.encode_images_device(cuda(block), records, o)
    assert not j.debug_routes() & j.ROUTE_JPEG_IMAGES
    assert got == want


def test_dense_groups_at_quality_100():
    j = J()
    shapes = [(97, 53, RGB, "n"), (1537, 9, GRAY, "n"), (512, 16, RGB, "n"), (40, 40, GRAY, "n")]
    pixels = content(shapes, 300)
    for ss in (1, 0):
        o = opts(ss, 100)
        block, records = lay_out(shapes, pixels, lead=2, gap=1)
        assert j.encode_images_device(cuda(block), records, o) == singles(shapes, pixels, o)


# ---- 2. alignment, what lies between the images -----------------------------------------------------------------------------------

ALIGNMENT = [BASIC[2], BASIC[0]] + BASIC[3:] + [BASIC[1], (2, 5, GRAY, "n"), (3, 2, RGB, "n")]  # an aligned image first


def test_alignment_load_forms_and_fill():
    j = J()
    shapes = ALIGNMENT
    pixels = content(shapes, 400)
    o = opts(1)
    want = singles(shapes, pixels, o, key="alignment")
    forms_by_layout = []
    for lead in (0, 1, 2, 3):
        files = []
        for fill in (0x11, 0xEE):
            block, records = lay_out(shapes, pixels, lead=lead, gap=lead, fill=fill, align=1)
            d_block = cuda(block)
            files.append(j.encode_images_device(d_block, records, o))
        assert files[0] == files[1], "the bytes between the images changed a file"
        for i in range(len(shapes)):
            assert files[0][i] == want[i], (i, shapes[i], lead)
        plan = j.encode_images_plan(records, o, alignment=d_block.data_ptr() % 16)
        forms_by_layout.append(set(plan["load_form"]))
    assert any(forms == {0, 1, 2} for forms in forms_by_layout), forms_by_layout
    # 4:4:4 and gray rows at every lead as well, one fill
    o444 = opts(0)
    want444 = singles(shapes, pixels, o444)
    for lead in (1, 2):
        block, records = lay_out(shapes, pixels, lead=lead, fill=0xEE)
        assert j.encode_images_device(cuda(block), records, o444) == want444


# ---- 3. order and overlap ------------------------------------------------------------------------------------------------------

def test_order_and_overlap():
    j = J()
    pixels, o, want = basic(1)
    block, records = lay_out(BASIC, pixels, lead=1)
    d_block = cuda(block)
    twice = j.encode_images_device(d_block, [records[7], records[7], records[6], records[7]], o)
    assert twice[0] == twice[1] == twice[3] == want[7] and twice[2] == want[6]
    got = j.encode_images_device(d_block, records[::-1], o)
    assert got == want[::-1]
    # an image inside another: the rows 10..29 of the 97 x 53 image
    w, h, ct, at = records[7]
    inner = (w, 20, ct, at + w * 3 * 10)
    got = j.encode_images_device(d_block, [records[7], inner], o)
    assert got[0] == want[7] and got[1] == j.encode_device(cuda(pixels[7][w * 3 * 10:w * 3 * 30]), for_image(o, w, 20, RGB))


# ---- 4. sub-batches ------------------------------------------------------------------------------------------------------------

def test_sub_batch_seams():
    j = J()
    pixels, o, want = basic(1)
    block, records = lay_out(BASIC, pixels, align=4)
    d_block = cuda(block)
    try:
        j.debug_configure("jpeg_images_blocks=400")
        plan = j.encode_images_plan(records, o)
        assert len(plan["sub_first"]) >= 4 and plan["sub_first"][0] == 0 and plan["sub_first"][-1] == len(BASIC), plan["sub_first"]
        j.debug_routes()
        got = j.encode_images_device(d_block, records, o)
        r = j.debug_routes()
    finally:
        j.debug_configure(None)
    assert got == want
    assert r & j.ROUTE_SUB_BATCHES and r & j.ROUTE_JPEG_IMAGES
    j.debug_routes()
    assert j.encode_images_device(d_block, records, o) == want and not j.debug_routes() & j.ROUTE_SUB_BATCHES


# ---- 5. many images, the same launches ------------------------------------------------------------------------------------------

def test_300_images_take_the_launches_of_6():
    j = J()
    first = [(8, 8, GRAY, "n"), (9, 8, GRAY, "n"), (8, 9, RGB, "n"), (9, 9, RGB, "n"), (40, 40, RGB, "n"), (40, 39, GRAY, "n")]
    rng = np.random.RandomState(5)
    shapes = first + [(int(rng.randint(8, 41)), int(rng.randint(8, 41)), (GRAY, RGB)[int(rng.randint(2))], "n") for _ in range(294)]
    sizes = [w * h * (ct + 1) for w, h, ct, _ in shapes]
    pixels = np.split(synth.lcg_bytes(sum(sizes), 500), np.cumsum(sizes)[:-1])  # (one stream of noise, cut into the images)
    o = opts(1)
    block, records = lay_out(shapes, pixels, align=4)
    d_block = cuda(block)
    six, all_of_them = j.encode_images_plan(records[:6], o), j.encode_images_plan(records, o)
    assert six["coef_launches"] == all_of_them["coef_launches"] == 4 and six["entropy_passes"] == all_of_them["entropy_passes"] == 2
    assert all(all_of_them["way_in"]) and all_of_them["sub_first"] == [0, 300]
    got = j.encode_images_device(d_block, records, o)
    for i, (w, h, ct, _) in enumerate(shapes):
        assert got[i] == j.encode_device(cuda(pixels[i]), for_image(o, w, h, ct)), (i, shapes[i])


# ---- 6. sinks ------------------------------------------------------------------------------------------------------------------

def test_into_arena_size_query_and_refusals():
    import torch
    from pixo_amd.error import BufferTooSmall, Error as PixoError
    j = J()
    pixels, o, want = basic(1)
    block, records = lay_out(BASIC, pixels, lead=1, gap=2)
    d_block = cuda(block)
    n = len(BASIC)
    offsets, lens = j.encode_images_device_into(None, d_block, records, o)  # the size query
    assert lens == [len(f) for f in want] and offsets == [sum(lens[:i]) for i in range(n)] and offsets[0] == 0
    total = offsets[-1] + lens[-1]
    for arena in (torch.full((total,), 0xEE, dtype=torch.uint8).pin_memory(), np.full(total, 0xEE, np.uint8)):  # exact size: pinned, pageable
        assert j.encode_images_device_into(arena, d_block, records, o) == (offsets, lens)
        flat = arena.numpy() if hasattr(arena, "numpy") else arena
        assert [flat[a:a + k].tobytes() for a, k in zip(offsets, lens)] == want
    short = np.full(total - 1, 0xEE, np.uint8)
    with pytest.raises(BufferTooSmall) as e:
        j.encode_images_device_into(short, d_block, records, o)
    assert str(e.value) == "output buffer too small: need %d bytes" % total
    assert (e.value.offsets, e.value.lens, e.value.needed) == (offsets, lens, total)
    with pytest.raises(PixoError):  # a device arena is refused
        j.encode_images_device_into(torch.zeros(total, dtype=torch.uint8, device="cuda"), d_block, records, o)
    assert j.encode_images_device(d_block, records, o) == want  # the next call on the same thread
    # the single way into an arena
    o1 = opts(preset=1)
    few, few_px = BASIC[:3] + BASIC[8:10], pixels[:3] + pixels[8:10]
    block1, records1 = lay_out(few, few_px)
    want1 = singles(few, few_px, o1)
    offsets1, lens1 = j.encode_images_device_into(None, cuda(block1), records1, o1)
    assert lens1 == [len(f) for f in want1]
    arena = np.zeros(sum(lens1), np.uint8)
    assert j.encode_images_device_into(arena, cuda(block1), records1, o1) == (offsets1, lens1)
    assert [arena[a:a + k].tobytes() for a, k in zip(offsets1, lens1)] == want1


def test_host_entry():
    from pixo_amd.error import InvalidDataLength
    j = J()
    pixels, o, want = basic(1)
    block, records = lay_out(BASIC, pixels, lead=3, gap=1)
    assert j.encode_images(block, records, o) == want
    assert j.encode_images(block.tobytes(), records, o) == want
    end = max(at + w * h * (int(ct) + 1) for w, h, ct, at in records)
    assert j.encode_images(block[:end], records, o) == want
    with pytest.raises(InvalidDataLength) as e:
        j.encode_images(block[:end - 1], records, o)
    assert str(e.value) == "Invalid pixel data length: expected %d bytes, got %d" % (end, end - 1)


# ---- 7. the chain: decode batch -> fit -> resize images -> JPEG images -----------------------------------------------------------

def test_chain_decode_fit_resize_encode():
    from pixo_amd import ColorType, decode, png, resize
    j = J()
    sources = [(97, 53, RGB), (64, 80, GRAY), (120, 30, RGB), (33, 47, GRAY)]
    files = []
    for i, (w, h, ct) in enumerate(sources):
        px = synth.scene(w, h, 600 + i).reshape(h, w, 3)
        px = px.reshape(-1) if ct == RGB else np.ascontiguousarray(px[:, :, 1]).reshape(-1)
        files.append(png.encode(px, png.PngOptions.builder(w, h).color_type(ColorType(ct)).preset(0).build()))
    views = decode.decode_png_batch_device(files)
    fitted, total = resize.fit_images(views, 48, 48)
    import torch
    d_dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    resize.resize_images_device(None, views, d_dst, fitted, resize.ResizeAlgorithm.Bilinear)
    torch.cuda.synchronize()
    o = opts(1)
    j.debug_routes()
    got = j.encode_images_device(d_dst, fitted, o)
    assert j.debug_routes() & j.ROUTE_JPEG_IMAGES
    host = d_dst.cpu().numpy()
    assert len(got) == 4
    for i, rec in enumerate(fitted):
        w, h, ct, at = (rec.width, rec.height, rec.color_type, rec.offset) if hasattr(rec, "width") else rec
        assert max(w, h) <= 48 and int(ct) == sources[i][2]
        alone = host[at:at + w * h * (int(ct) + 1)]
        assert got[i] == j.encode_device(cuda(alone), for_image(o, w, h, int(ct))), i


# ---- 8. an independent decoder -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ss", [1, 0], ids=["420", "444"])
def test_files_decode_with_pillow(ss):
    from PIL import Image
    j = J()
    pixels, o, _ = basic(ss)
    block, records = lay_out(BASIC, pixels, lead=1)
    got = j.encode_images_device(cuda(block), records, o)
    for blob, (w, h, ct, _) in zip(got, BASIC):
        im = Image.open(io.BytesIO(blob))
        im.load()
        assert im.size == (w, h) and im.mode == ("L" if ct == GRAY else "RGB"), (w, h, ct)


# ---- 9. long segments: the block sums of the two-level look-back -----------------------------------------------------------------
# From here on the expectation of a file is the oracle's, and the single entry's file is held against it in the same test.
# The shapes come from tests/jpeg_images_cases.py by group count; every test asserts the counts from the plan entry.

_LONG_PIXELS, _LONG_ORACLE, _LONG_SINGLE = {}, {}, {}


def long_pixels(ss):
    if ss not in _LONG_PIXELS:
        shapes, claimed = K.long_list(ss)
        _LONG_PIXELS[ss] = (shapes, claimed, K.make_pixels(shapes, 700))
    return _LONG_PIXELS[ss]


def long_expected(ss, q, idx):
    """the oracle's files for images idx of the long list, each computed once; the single entry's file for the same image
    (uploaded alone) is held against it when it is made"""
    shapes, _, pixels = long_pixels(ss)
    o = opts(ss, q)
    for i in idx:
        if (ss, q, i) not in _LONG_ORACLE:
            w, h, ct, _ = shapes[i]
            _LONG_ORACLE[ss, q, i] = O.encode(pixels[i], O.make_options(w, h, ct, q, ss))
            _LONG_SINGLE[ss, q, i] = J().encode_device(cuda(pixels[i]), for_image(o, w, h, ct))
        assert _LONG_SINGLE[ss, q, i] == _LONG_ORACLE[ss, q, i], ("the single entry against the oracle", ss, q, i, shapes[i])
    return [_LONG_ORACLE[ss, q, i] for i in idx]


def long_call(ss, q, idx, **layout):
    """-> (device block, records, the groups the plan entry gives them, the oracle's files) for images idx of the long list"""
    shapes, claimed, pixels = long_pixels(ss)
    block, records = K.lay_out(shapes, pixels, idx, **layout)
    groups = K.plan_groups(J(), records, opts(ss, q))
    assert groups == [claimed[i] for i in idx], "the shapes do not have the groups the test is about"
    return cuda(block), records, groups, long_expected(ss, q, idx)


def scan_bytes(blob):
    """the entropy-coded bytes of a baseline file: behind the SOS segment, in front of EOI"""
    at = blob.index(b"\xff\xda")
    return len(blob) - (at + 2 + int.from_bytes(blob[at + 2:at + 4], "big")) - 2


@pytest.mark.parametrize("ss", [1, 0], ids=["420", "444"])
def test_long_segments_read_and_write_block_sums(ss):
    """Segments of 1, 65, 64, 129, 1, 63 and 66-68 groups per colour class, gray and RGB interleaved: floors that are no
    multiples of 64, groups that read one and two block sums, the 64th group that writes one nobody reads, 390 groups a pass
    (the sums in 16 copies); in list order, reversed, and with the 65-group images in front (their words end where the next
    segment's begin)."""
    j = J()
    n = len(long_pixels(ss)[0])
    fallbacks = j.lookback_fallbacks()
    for which in K.ORDERS:
        idx = K.order(n, which)
        layout = dict(lead=1, gap=1) if which == "reversed" else dict(align=16)  # (reversed: rows at any address as well)
        d_block, records, groups, want = long_call(ss, 80, idx, **layout)
        per_class = {ct: [g for g, r in zip(groups, records) if int(r[2]) == ct] for ct in (GRAY, RGB)}
        assert all(sum(per) >= 256 and max(per) == 129 for per in per_class.values()), per_class
        if which == "tight":
            assert all(per[0] == 65 for per in per_class.values())
        elif which == "list":
            assert all(per[:6] == [1, 65, 64, 129, 1, 63] for per in per_class.values())
        j.debug_routes()
        got = j.encode_images_device(d_block, records, opts(ss, 80))
        r = j.debug_routes()
        for k, i in enumerate(idx):
            assert got[k] == want[k], (which, k, i, records[k], groups[k])
        assert r & j.ROUTE_JPEG_IMAGES and not r & j.ROUTE_FALLBACK and not r & j.ROUTE_SUB_BATCHES, hex(r)
        assert j.lookback_fallbacks() == fallbacks


def test_a_segment_of_more_than_4096_groups_among_short_ones():
    """look_back_blocks' second round of block sums (64 sums a round): 4097 groups at 4:4:4 behind a one-group image and in
    front of a 65-group one.  The yardstick is the single entry alone (held against the oracle at 4096 x 4096 by
    test_gpu_parity); the content is 1 MiB + 13 bytes of noise repeated."""
    j = J()
    shapes = [(40, 40, RGB, "n"), (512, 8 * 4097, RGB, "n"), (520, 512, RGB, "n"), (40, 40, GRAY, "n")]
    noise = synth.lcg_bytes((1 << 20) + 13, 900)
    pixels = [np.resize(noise[i:], w * h * (ct + 1)) for i, (w, h, ct, _) in enumerate(shapes)]
    o = opts(0)
    block, records = lay_out(shapes, pixels, align=16)
    assert K.plan_groups(j, records, o) == [1, 4097, 65, 1]
    want = singles(shapes, pixels, o)
    fallbacks = j.lookback_fallbacks()
    j.debug_routes()
    got = j.encode_images_device(cuda(block), records, o)
    r = j.debug_routes()
    assert [len(f) for f in got] == [len(f) for f in want]
    assert got == want
    assert r & j.ROUTE_JPEG_IMAGES and not r & j.ROUTE_FALLBACK and j.lookback_fallbacks() == fallbacks


# ---- 10. the packed forms of the ragged coefficient kernel -------------------------------------------------------------------------

@pytest.mark.parametrize("ss", [1, 0], ids=["420", "444"])
def test_packed_coefficient_forms_by_switch(ss):
    """jpeg_images_coeffs_kernel<MODE, LOAD, true> for all three load forms x gray / RGB: the alignment set under
    coef_form=packed against the oracle"""
    j = J()
    shapes = ALIGNMENT
    pixels = content(shapes, 400)
    want = [O.encode(px, O.make_options(w, h, ct, 80, ss)) for (w, h, ct, _), px in zip(shapes, pixels)]
    o = opts(ss)
    try:
        j.debug_configure("coef_form=packed")
        seen = set()
        for lead in (0, 1, 2, 3):
            block, records = lay_out(shapes, pixels, lead=lead, gap=lead, fill=0xEE)
            d_block = cuda(block)
            plan = j.encode_images_plan(records, o, alignment=d_block.data_ptr() % 16)
            seen |= {(int(rec[2]), form) for rec, form in zip(records, plan["load_form"])}
            j.debug_routes()
            got = j.encode_images_device(d_block, records, o)
            r = j.debug_routes()
            for i in range(len(shapes)):
                assert got[i] == want[i], (i, shapes[i], lead)
            assert r & j.ROUTE_COEF_PACKED and not r & j.ROUTE_COEF_SCALAR and r & j.ROUTE_JPEG_IMAGES, hex(r)
        assert seen == {(ct, form) for ct in (GRAY, RGB) for form in (0, 1, 2)}, seen
    finally:
        j.debug_configure(None)
    j.debug_routes()
    block, records = lay_out(shapes, pixels)
    assert j.encode_images_device(cuda(block), records, o) == want
    r = j.debug_routes()
    assert r & j.ROUTE_COEF_SCALAR and not r & j.ROUTE_COEF_PACKED, hex(r)


def test_packed_coefficient_forms_by_size():
    """more than 2048 tiles in one launch (2100 gray images of one tile each, aligned) take the packed forms by themselves;
    the launches of the few other images beside them stay scalar"""
    from pixo_amd import ColorType
    j = J()
    distinct = [synth.lcg_bytes(64, 1000 + k) for k in range(4)] + [np.full(64, 255, np.uint8)]
    others = [(16, 16, RGB, "n"), (7, 9, GRAY, "n"), (97, 53, RGB, "n"), (2, 5, GRAY, "n"), (9, 9, RGB, "n")]
    other_px = content(others, 1100)
    n_tiles = 2100
    records, parts, at, kind = [], [], 0, []
    for i in range(n_tiles + len(others)):
        if i % 500 == 100:  # (the other classes spread over the call: images 100, 600, 1100, 1600 and 2100)
            k = i // 500
            w, h, ct, _ = others[k]
            px = other_px[k]
            kind.append(5 + k)
        else:
            w, h, ct = 8, 8, GRAY
            px = distinct[i % 5]
            kind.append(i % 5)
        at = -(-at // 16) * 16
        records.append((w, h, ColorType(ct), at))
        parts.append((at, px))
        at += px.size
    assert sum(k < 5 for k in kind) > 2048 and sorted(k for k in kind if k >= 5) == [5, 6, 7, 8, 9]
    block = np.full(at + 16, 0x11, np.uint8)
    for off, px in parts:
        block[off:off + px.size] = px
    want_of = {k: O.encode(distinct[k], O.make_options(8, 8, GRAY, 80, 1)) for k in range(5)}
    for k, ((w, h, ct, _), px) in enumerate(zip(others, other_px)):
        want_of[5 + k] = O.encode(px, O.make_options(w, h, ct, 80, 1))
    o = opts(1)
    d_block = cuda(block)
    plan = j.encode_images_plan(records, o, alignment=d_block.data_ptr() % 16)
    assert all(plan["way_in"]) and plan["sub_first"] == [0, len(records)]
    assert all(form == 0 for form, k in zip(plan["load_form"], kind) if k < 5)  # one launch: gray, aligned, one tile an image
    assert j.encode_device(cuda(distinct[0]), for_image(o, 8, 8, GRAY)) == want_of[0]
    j.debug_routes()
    got = j.encode_images_device(d_block, records, o)
    r = j.debug_routes()
    wrong = [i for i, k in enumerate(kind) if got[i] != want_of[k]]
    assert not wrong, (len(wrong), wrong[:8])
    assert r & j.ROUTE_COEF_PACKED and r & j.ROUTE_COEF_SCALAR and r & j.ROUTE_JPEG_IMAGES, hex(r)
    assert not r & j.ROUTE_JPEG_IMAGES_DIRECT


# ---- 11. the sinks at file sizes that take the direct copies, the retries of the stuffing pass ------------------------------------------
# Noise at quality 100 from the long list: the 1-, 65-, 63- and 66-68-group RGB images, the 1-, 65- and 64-group gray ones.
DENSE = [0, 1, 2, 3, 5, 10, 12]
DIRECT_FROM = 4 << 20  # (the scans of a call of fewer than 128 images)


def dense_call(ss):
    d_block, records, groups, want = long_call(ss, 100, DENSE, align=4)
    assert sum(scan_bytes(f) for f in want) >= DIRECT_FROM and len(DENSE) < 128
    return d_block, records, want


@pytest.mark.parametrize("ss", [1, 0], ids=["420", "444"])
def test_short_guesses_grow_after_trim_and_large_files_travel_directly(ss):
    """After trim() the stuffed scans' buffer starts at a quarter of the stream bound (52 bytes a block, 65 with headroom) and
    the stuffing grid at 64 bytes a block; noise at quality 100 has 84-101: both fall short, RESTUFF_GROW is noted; the same
    call again finds the room.  The files, 1 MB each, go by the direct copies into pool blocks."""
    j = J()
    d_block, records, want = dense_call(ss)
    o = opts(ss, 100)
    j.trim()
    j.debug_routes()
    got = j.encode_images_device(d_block, records, o)
    r = j.debug_routes()
    assert got == want
    assert sum(scan_bytes(f) for f in got) >= DIRECT_FROM
    assert r & j.ROUTE_RESTUFF_GROW and r & j.ROUTE_JPEG_IMAGES and r & j.ROUTE_JPEG_IMAGES_DIRECT and not r & j.ROUTE_FALLBACK, hex(r)
    got = j.encode_images_device(d_block, records, o)
    r = j.debug_routes()
    assert got == want
    assert not r & j.ROUTE_RESTUFF_GROW and r & j.ROUTE_JPEG_IMAGES_DIRECT, hex(r)


@pytest.mark.parametrize("ss", [1, 0], ids=["420", "444"])
def test_sinks_of_large_files(ss):
    import torch
    from pixo_amd.error import BufferTooSmall
    j = J()
    d_block, records, want = dense_call(ss)
    o = opts(ss, 100)
    lens = [len(f) for f in want]
    offsets = [sum(lens[:i]) for i in range(len(lens))]
    total = sum(lens)

    def files_in(flat):
        return [flat[a:a + k].tobytes() for a, k in zip(offsets, lens)]

    j.debug_routes()
    assert j.encode_images_device_into(None, d_block, records, o) == (offsets, lens)  # the size query copies nothing
    assert not j.debug_routes() & j.ROUTE_JPEG_IMAGES_DIRECT
    assert sum(k - (len(f) - scan_bytes(f)) for k, f in zip(lens, want)) >= DIRECT_FROM  # (from the returned lengths)
    # pooled blocks
    assert j.encode_images_device(d_block, records, o) == want
    assert j.debug_routes() & j.ROUTE_JPEG_IMAGES_DIRECT
    # a pinned arena of exactly the size
    arena = torch.full((total,), 0xEE, dtype=torch.uint8).pin_memory()
    assert j.encode_images_device_into(arena, d_block, records, o) == (offsets, lens)
    assert j.debug_routes() & j.ROUTE_JPEG_IMAGES_DIRECT
    assert files_in(arena.numpy()) == want
    # a pinned arena with sentinel bytes behind
    arena = torch.full((total + 64,), 0xEE, dtype=torch.uint8).pin_memory()
    assert j.encode_images_device_into(arena[:total], d_block, records, o) == (offsets, lens)
    assert j.debug_routes() & j.ROUTE_JPEG_IMAGES_DIRECT
    assert files_in(arena.numpy()) == want and (arena.numpy()[total:] == 0xEE).all()
    # a pageable arena: through the context's pinned buffer
    pageable = np.full(total + 64, 0xEE, np.uint8)
    assert j.encode_images_device_into(pageable[:total], d_block, records, o) == (offsets, lens)
    r = j.debug_routes()
    assert r & j.ROUTE_JPEG_IMAGES and not r & j.ROUTE_JPEG_IMAGES_DIRECT, hex(r)
    assert files_in(pageable) == want and (pageable[total:] == 0xEE).all()
    # one byte short, pinned and pageable: the sizes, and nothing behind the capacity
    arena = torch.full((total + 64,), 0xEE, dtype=torch.uint8).pin_memory()
    for short in (arena.numpy(), np.full(total + 64, 0xEE, np.uint8)):
        with pytest.raises(BufferTooSmall) as e:
            j.encode_images_device_into(short[:total - 1], d_block, records, o)
        assert (e.value.offsets, e.value.lens, e.value.needed) == (offsets, lens, total)
        assert (short[total - 1:] == 0xEE).all()
    j.debug_routes()
    # small files never take the direct copies
    pixels, o80, small = basic(1)
    block, small_records = lay_out(BASIC, pixels, align=16)
    assert j.encode_images_device(cuda(block), small_records, o80) == small
    r = j.debug_routes()
    assert r & j.ROUTE_JPEG_IMAGES and not r & j.ROUTE_JPEG_IMAGES_DIRECT, hex(r)


# ---- 12. call history on one context ---------------------------------------------------------------------------------------------

def test_call_history_on_one_context():
    """The words of the coding pass's state (descriptors, tails, block sums) are left zero by the stuffing kernel and known to
    be (`e_code_state.known`); the single, batch and images entries lay them out differently.  One thread: small images, the
    long list, small, one 1024 x 512 image by the single entry, four 333 x 77 images by the batch entry, the long list at the
    other subsampling with the 65-group images in front, small.  Every result against the oracle."""
    j = J()
    pixels, o, _ = basic(1)
    small = [O.encode(px, O.make_options(w, h, ct, 80, 1)) for (w, h, ct, _), px in zip(BASIC, pixels)]
    small_block, small_records = lay_out(BASIC, pixels, align=16)
    d_small = cuda(small_block)
    n = len(long_pixels(1)[0])
    first = long_call(1, 80, K.order(n, "list"), align=16)
    second = long_call(0, 80, K.order(n, "tight"), align=16)
    one = synth.lcg_bytes(1024 * 512 * 3, 1200)
    one_want = O.encode(one, O.make_options(1024, 512, RGB, 80, 0))
    four = [synth.lcg_bytes(333 * 77 * 3, 1300 + i) for i in range(4)]
    four_want = [O.encode(px, O.make_options(333, 77, RGB, 80, 1)) for px in four]
    d_one, d_four = cuda(one), cuda(np.concatenate(four))
    fallbacks = j.lookback_fallbacks()
    j.debug_routes()

    def small_call(step):
        assert j.encode_images_device(d_small, small_records, o) == small, step

    def long_one(step, ss, call):
        d_block, records, _, want = call
        got = j.encode_images_device(d_block, records, opts(ss))
        assert [i for i in range(len(want)) if got[i] != want[i]] == [], step

    small_call(0)
    long_one(1, 1, first)
    small_call(2)
    assert j.encode_device(d_one, for_image(opts(0), 1024, 512, RGB)) == one_want
    assert j.encode_batch_device(d_four, for_image(opts(1), 333, 77, RGB), 4) == four_want
    long_one(5, 0, second)
    small_call(6)
    long_one(7, 1, first)
    r = j.debug_routes()
    assert r & j.ROUTE_JPEG_IMAGES and not r & j.ROUTE_FALLBACK and j.lookback_fallbacks() == fallbacks
