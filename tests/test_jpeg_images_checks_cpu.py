"""CPU-only: the JPEG encode entries for images of individual sizes (pixo_hip_jpeg_encode_images*): symbols, the route bit, the
argument checks in the documented order — status and exact pixo_hip_last_error() text, " (image i)" included; every check runs
before the thread's context is touched — and the plan (way in, load form, first group, sub-batches, launches) against values
worked out here.
Order: null options, the template's quality and Some(0) restart interval, null pixels, null images, batch in 1..65535, null
files / offsets, null lens, then image by image: zero side, side above 65535, a colour type that is not Gray or Rgb, offset +
bytes beyond 2^62; the host entry last: data_len below the furthest image's end."""
import ctypes as C
import os
import re

import pytest

from pixo_amd import ColorType, _lib, decode, jpeg, png, resize
from test_entry_checks_cpu import COLOUR, COMPRESSION, DIMS, LARGE, LENGTH, P, UNSUPPORTED, dims, large, last_error, length, null, run

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NAMES = ("pixo_hip_jpeg_encode_images_device", "pixo_hip_jpeg_encode_images_device_into", "pixo_hip_jpeg_encode_images",
         "pixo_hip_debug_jpeg_encode_images_plan")
QUALITY, RESTART = -3, -7
BATCH = "Compression error: batch must be 1..65535"
TOO_FAR = "Compression error: batch input too large"
GRAY, GA, RGB, RGBA = 0, 1, 2, 3
SIDE = 65535


def test_symbols_are_declared_listed_and_exported():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pixo_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name


def test_route_bit_is_new():
    routes = open(os.path.join(ROOT, "pixo_amd", "csrc", "routes.hpp")).read()
    assert re.search(r"\bRESIZE_IMAGES = 1ull << 47,", routes) and re.search(r"\bJPEG_IMAGES = RESIZE_IMAGES << 1,", routes)  # bit 48
    assert re.search(r"\bJPEG_IMAGES_DIRECT = JPEG_IMAGES << 1,", routes)  # bit 49: the direct copies of large files
    assert jpeg.IMAGES_ROUTES == {"JPEG_IMAGES": 48, "JPEG_IMAGES_DIRECT": 49}
    assert jpeg.ROUTE_JPEG_IMAGES == 1 << 48 and jpeg.ROUTE_JPEG_IMAGES_DIRECT == 1 << 49
    taken = set(png.ROUTES.values()) | set(png.IMAGES_ROUTES.values()) | set(jpeg.ROUTES.values()) | set(decode.ROUTES.values()) | \
        set(decode.INFLATE_ROUTES.values()) | set(resize.ROUTES.values())
    assert 48 not in taken and 49 not in taken


def images_c(*rows):
    """rows of (width, height, colour type, offset)"""
    arr = (_lib.PngImageC * max(len(rows), 1))()
    for i, (w, h, ct, at) in enumerate(rows):
        arr[i].width, arr[i].height, arr[i].color_type, arr[i].offset = w, h, ct, at
    return arr


GOOD = ((4, 4, RGB, 0), (5, 3, GRAY, 64))  # 48 bytes at 0, 15 bytes at 64: the block ends at 79


def options_c(quality=80, restart=None, w=0, h=0, ct=9):
    """(width 0, height 0 and a colour type that is none: the template's own are not read)"""
    return _lib.JpegOptionsC(w, h, ct, quality, 1, 0 if restart is None else 1, restart or 0, 0, 0, 0)


def shared_rows(sink):
    far = 1 << 62
    return [
        (dict(o=None, pixels=None), COMPRESSION, null("options")),
        (dict(quality=0, restart=0, pixels=None), QUALITY, "Invalid quality 0: must be 1-100"),  # the quality before the restart interval
        (dict(quality=101, pixels=None), QUALITY, "Invalid quality 101: must be 1-100"),
        (dict(restart=0, pixels=None), RESTART, "Invalid restart interval 0: must be 1-65535 (or None to disable)"),  # the template before the pixels
        (dict(pixels=None, images=None), COMPRESSION, null("d_pixels")),  # pixels before images
        (dict(images=None, batch=0), COMPRESSION, null("images")),  # images before batch
        (dict(batch=0, **{sink: None}), COMPRESSION, BATCH),  # batch before the sink
        (dict(batch=65536), COMPRESSION, BATCH),
        (dict(**{sink: None}, lens=None), COMPRESSION, null(sink)),  # files / offsets before lens
        (dict(lens=None, images=((0, 4, RGB, 0),), batch=1), COMPRESSION, null("lens")),  # lens before the images' own
        (dict(images=((4, 4, RGB, 0), (0, SIDE + 1, 9, far)), batch=2), DIMS, dims(0, SIDE + 1) + " (image 1)"),  # a zero side first
        (dict(images=((4, 0, RGB, 0), (0, 4, RGB, 0)), batch=2), DIMS, dims(4, 0) + " (image 0)"),  # the lowest index decides
        (dict(images=((4, 4, GRAY, 0), (SIDE + 1, 1, RGBA, 0), (0, 1, RGB, 0)), batch=3), LARGE, large(SIDE + 1, 1, SIDE) + " (image 1)"),  # ... also when a later image fails differently
        (dict(images=((SIDE + 1, 1, 9, far),), batch=1), LARGE, large(SIDE + 1, 1, SIDE) + " (image 0)"),  # too large before the colour type
        (dict(images=((4, 4, RGB, 0), (4, 4, GRAY, 0), (1, SIDE + 1, RGB, 0)), batch=3), LARGE, large(1, SIDE + 1, SIDE) + " (image 2)"),
        (dict(images=((4, 4, RGBA, far),), batch=1), COLOUR, UNSUPPORTED + " (image 0)"),  # the colour type before the offset; RGBA is refused
        (dict(images=((4, 4, RGB, 0), (4, 4, GA, 0)), batch=2), COLOUR, UNSUPPORTED + " (image 1)"),  # GrayAlpha too
        (dict(images=((4, 4, RGB, 0), (4, 4, 4, 0)), batch=2), COLOUR, UNSUPPORTED + " (image 1)"),  # a colour type above 3
        (dict(images=((4, 4, RGB, 0), (4, 4, 255, 0)), batch=2), COLOUR, UNSUPPORTED + " (image 1)"),
        (dict(images=((4, 4, RGB, far - 47),), batch=1), COMPRESSION, TOO_FAR + " (image 0)"),  # 48 bytes: one beyond 2^62
        (dict(images=((4, 4, RGB, 0), (4, 4, GRAY, (1 << 64) - 8)), batch=2), COMPRESSION, TOO_FAR + " (image 1)"),  # (no wrap)
    ]


def entry(fn):
    def call(o=(), quality=80, restart=None, images=GOOD, batch=None, **kw):
        oc = options_c(quality, restart) if o is not None else None
        arr = images_c(*images) if images is not None else None
        n = batch if batch is not None else (len(images) if images is not None else 2)
        return fn(C.byref(oc) if oc is not None else None, arr, n, **kw)
    return call


def test_jpeg_encode_images_device():
    L = _lib.load()
    files, lens = (C.POINTER(C.c_uint8) * 3)(), (C.c_size_t * 3)()

    @entry
    def call(o, images, batch, pixels=P, files=files, lens=lens):
        return L.pixo_hip_jpeg_encode_images_device(pixels, images, batch, o, files, lens)

    run(shared_rows("files"), call)
    assert not files[0] and not files[1] and lens[0] == 0


def test_jpeg_encode_images_device_into():
    L = _lib.load()
    offsets, lens = (C.c_size_t * 3)(), (C.c_size_t * 3)()

    @entry
    def call(o, images, batch, pixels=P, arena=P, cap=4096, offsets=offsets, lens=lens):
        return L.pixo_hip_jpeg_encode_images_device_into(pixels, images, batch, o, arena, cap, offsets, lens)

    run(shared_rows("offsets"), call)


def test_jpeg_encode_images_host():
    L = _lib.load()
    files, lens = (C.POINTER(C.c_uint8) * 3)(), (C.c_size_t * 3)()

    @entry
    def call(o, images, batch, pixels=P, n=4096, files=files, lens=lens):
        return L.pixo_hip_jpeg_encode_images(pixels, n, images, batch, o, files, lens)

    rows = [(kw, rc, text.replace("'d_pixels'", "'data'")) for kw, rc, text in shared_rows("files")]
    run(rows + [
        (dict(n=78), LENGTH, length(79, 78)),  # the furthest image's end, behind every image's own checks
        (dict(n=0, images=((4, 4, RGB, 100), (5, 3, GRAY, 0))), LENGTH, length(148, 0)),  # (the furthest, not the last)
        (dict(n=78, images=((4, 4, RGB, 0), (5, 3, GRAY, 64), (4, 4, RGBA, 0)), batch=3), COLOUR, UNSUPPORTED + " (image 2)"),
    ], call)


def plan_call(images, o, alignment=0, drop=None):
    L = _lib.load()
    n = len(images)
    outs = dict(sub_first=(C.c_uint32 * (n + 1))(), sub_count=C.byref(C.c_uint32()), way_in=(C.c_uint8 * n)(), load_form=(C.c_uint8 * n)(),
                first_group=(C.c_uint64 * n)(), coef_launches=C.byref(C.c_uint32()), entropy_passes=C.byref(C.c_uint32()))
    if drop:
        outs[drop] = None
    return L.pixo_hip_debug_jpeg_encode_images_plan(images_c(*images), n, C.byref(o) if o is not None else None, alignment, *outs.values())


def test_plan_checks():
    assert plan_call(GOOD, None) == COMPRESSION and last_error() == null("options")
    assert plan_call(GOOD, options_c(quality=0), alignment=16) == QUALITY
    assert plan_call(GOOD, options_c(), alignment=16) == COMPRESSION and last_error() == "Compression error: alignment must be 0..15"
    for name in ("sub_first", "sub_count", "way_in", "load_form", "first_group", "coef_launches", "entropy_passes"):
        assert plan_call(GOOD, options_c(), drop=name) == COMPRESSION and last_error() == null(name), name
    assert plan_call(((4, 4, RGB, 0), (4, 4, RGBA, 0)), options_c()) == COLOUR and last_error() == UNSUPPORTED + " (image 1)"
    assert plan_call(GOOD, options_c()) == 0


# ---- the plan ----------------------------------------------------------------------------------------------------------------

def template(ss=1, q=80, preset=None, restart=None):
    b = jpeg.JpegOptions.builder(0, 0).quality(q)
    if preset is not None:
        return b.preset(preset).build()
    b = b.subsampling(jpeg.Subsampling(ss))
    return (b.restart_interval(restart) if restart is not None else b).build()


def blocks(w, h, ct, ss):
    unit = 16 if ct == RGB and ss == 1 else 8
    units = -(-w // unit) * -(-h // unit)
    return units if ct == GRAY else (6 * units if ss == 1 else 3 * units)


SIX = [(8, 8, ColorType.Gray, 0), (9, 8, ColorType.Gray, 64), (8, 9, ColorType.Rgb, 256), (9, 9, ColorType.Rgb, 512), (3, 40, ColorType.Rgb, 1024),
       (1537, 9, ColorType.Gray, 2048)]


def test_plan_way_in_per_preset():
    assert jpeg.encode_images_plan(SIX, template(preset=0))["way_in"] == [True] * 6
    for preset in (1, 2):
        p = jpeg.encode_images_plan(SIX, template(preset=preset))
        assert p["way_in"] == [False] * 6 and p["coef_launches"] == 0 and p["entropy_passes"] == 0 and p["first_group"] == [0] * 6
        assert p["sub_first"] == [0, 6]
    assert jpeg.encode_images_plan(SIX, jpeg.JpegOptions.builder(0, 0).progressive(True).build())["way_in"] == [False] * 6
    # restart markers: only where the interval is below the image's MCUs (the single entry's rule); a sub-batch ends where the way changes
    p = jpeg.encode_images_plan(SIX, template(ss=0, restart=2))
    assert p["way_in"] == [True, True, True, False, False, False] and p["sub_first"] == [0, 3, 6]  # one or two MCUs: no marker is written
    assert jpeg.encode_images_plan(SIX, template(ss=0, restart=65535))["way_in"] == [True] * 6


def test_plan_load_form_by_alignment_and_width():
    o = template()
    records = [(8, 2, ColorType.Gray, 0), (7, 2, ColorType.Gray, 16), (3, 2, ColorType.Gray, 32), (4, 2, ColorType.Rgb, 48), (5, 2, ColorType.Rgb, 80),
               (1, 2, ColorType.Rgb, 112), (8, 2, ColorType.Gray, 130), (4, 4, ColorType.Rgb, 161)]
    assert jpeg.encode_images_plan(records, o, alignment=0)["load_form"] == [0, 1, 2, 0, 1, 2, 1, 1]
    assert jpeg.encode_images_plan(records, o, alignment=8)["load_form"] == [0, 1, 2, 0, 1, 2, 1, 1]
    assert jpeg.encode_images_plan(records, o, alignment=2)["load_form"] == [1, 1, 2, 1, 1, 2, 0, 1]  # (130 + 2 is a multiple of 4)
    assert jpeg.encode_images_plan(records, o, alignment=3)["load_form"] == [1, 1, 2, 1, 1, 2, 1, 0]  # (161 + 3 too)
    p = jpeg.encode_images_plan(records, o, alignment=0)
    assert p["coef_launches"] == 6 and p["entropy_passes"] == 2  # gray and RGB, each in all three forms


@pytest.mark.parametrize("ss", [1, 0])
def test_plan_first_group(ss):
    records = [(512, 16, ColorType.Rgb, 0), (7, 9, ColorType.Gray, 30000), (520, 8, ColorType.Rgb, 40000), (1537, 9, ColorType.Gray, 60000),
               (1, 1, ColorType.Rgb, 90000), (8, 8, ColorType.Gray, 90016), (97, 53, ColorType.Rgb, 90100)]
    want, at = [], {GRAY: 0, RGB: 0}
    for w, h, ct, _ in records:
        want.append(at[int(ct)])
        at[int(ct)] += -(-blocks(w, h, int(ct), ss) // 192)
    p = jpeg.encode_images_plan(records, template(ss))
    assert p["first_group"] == want
    if ss == 1:
        assert want == [0, 0, 1, 1, 3, 4, 4]  # 512x16 is exactly one group; 520x8 is 33 MCUs: two; 1537x9 gray 386 blocks: three
    else:
        assert want == [0, 0, 2, 1, 4, 4, 5]  # 512x16 at 4:4:4 is 384 blocks: two groups; 520x8 is 195: two


def test_plan_sub_batch_cuts_under_the_debug_switch():
    o = template()
    sizes = [blocks(w, h, int(ct), 1) for w, h, ct, _ in SIX]  # 1, 2, 6, 6, 18, 386
    assert sizes == [1, 2, 6, 6, 18, 386]
    try:
        jpeg.debug_configure("jpeg_images_blocks=9")
        p = jpeg.encode_images_plan(SIX, o)
        assert p["sub_first"] == [0, 3, 4, 5, 6]  # greedy: 1 + 2 + 6, then 6, then 18 and 386 by themselves (at least one image each)
        assert p["first_group"] == [0, 1, 0, 0, 0, 0] and p["coef_launches"] == 6 and p["entropy_passes"] == 5
        jpeg.debug_configure("jpeg_images_blocks=33")
        assert jpeg.encode_images_plan(SIX, o)["sub_first"] == [0, 5, 6]
    finally:
        jpeg.debug_configure(None)
    assert jpeg.encode_images_plan(SIX, o)["sub_first"] == [0, 6]


def test_plan_launches_follow_the_classes_not_the_batch():
    o = template()
    six = jpeg.encode_images_plan(SIX, o)
    sixty = jpeg.encode_images_plan(SIX * 10, o)
    assert six["coef_launches"] == sixty["coef_launches"] == 5  # gray aligned and funnel; RGB aligned, funnel and bytes
    assert six["entropy_passes"] == sixty["entropy_passes"] == 2
    assert sixty["sub_first"] == [0, 60] and all(sixty["way_in"])


def test_wrapper_refusals():
    with pytest.raises(Exception):
        jpeg.encode_images_plan([], template())
