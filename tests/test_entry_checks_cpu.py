"""CPU-only: the argument checks of every PNG, zlib and resize entry point of the C ABI, in the order each entry runs them.
Every check runs before the thread's context is touched, so none of these calls needs a device.  One ordered table per
entry: a row is a call with one defect, or with two so that the ORDER of the two checks is pinned, and asserts the status
and the exact pixo_hip_last_error() text.  The host layer behind these entries may be rearranged; this file may not notice."""
import ctypes as C

import numpy as np

from pixo_amd import _lib

OK, DIMS, LENGTH, LARGE, COLOUR, COMPRESSION, COLOUR_ARG, SMALL = 0, -1, -2, -4, -5, -6, -8, -9
MAX = 1 << 24
CALLER_RETRY = 1 << 13  # routes.hpp
SENTINEL = 0xABCDEF

BUF = np.zeros(4096, np.uint8)  # stands for every pointer a bad call never follows
P = BUF.ctypes.data

STRATEGY = "Compression error: unknown PNG filter strategy"
UNSUPPORTED = "Unsupported color type for this format"
BAD_COLOUR = "Invalid color type: %d. Expected 0 (Gray), 1 (GrayAlpha), 2 (Rgb), or 3 (Rgba)"
BAD_ALGORITHM = "Invalid resize algorithm: %d. Expected 0 (Nearest), 1 (Bilinear), or 2 (Lanczos3)"


def null(name):
    return "Compression error: null argument '%s'" % name


def length(want, got):
    return "Invalid pixel data length: expected %d bytes, got %d" % (want, got)


def dims(w, h):
    return "Invalid image dimensions: %dx%d" % (w, h)


def large(w, h, m=MAX):
    return "Image %dx%d exceeds maximum dimension %d" % (w, h, m)


def small(n, what="bytes"):
    return "output buffer too small: need %d %s" % (n, what)


def last_error():
    return _lib.load().pixo_hip_last_error().decode()


def routes():
    return _lib.load().pixo_hip_debug_routes(1)


def png_options(w=4, h=4, ct=3, strategy=7):
    return _lib.PngOptionsC(w, h, ct, strategy, 0, 0, 0, 2, 0, 0, 0)


def resize_options(sw=4, sh=4, dw=2, dh=2, ct=3, alg=2):
    return _lib.ResizeOptionsC(sw, sh, dw, dh, ct, alg)


def run(table, call):
    """Every row of an ordered table: (keyword overrides of the entry's good call, status, last error)."""
    for i, (kw, status, message) in enumerate(table):
        assert call(**kw) == status, (i, kw, last_error())
        assert last_error() == message, (i, kw)


# ---- the options entries: zero dimension < too large < colour type < data length < unknown strategy < nulls ----------
# (`o`: pixo_png_options fields as a tuple w, h, colour type, strategy; None: a null options pointer)
PNG_OPTION_ROWS = [
    (dict(o=None), COMPRESSION, null("o")),
    (dict(o=(0, MAX + 1, 9, 9), n=1), DIMS, dims(0, MAX + 1)),
    (dict(o=(MAX + 1, 0, 3, 7)), DIMS, dims(MAX + 1, 0)),
    (dict(o=(MAX + 1, 1, 9, 9), n=1), LARGE, large(MAX + 1, 1)),
    (dict(o=(1, MAX + 1, 3, 7)), LARGE, large(1, MAX + 1)),
    (dict(o=(4, 4, 4, 9), n=1), COLOUR, UNSUPPORTED),
    (dict(o=(4, 4, 255, 7)), COLOUR, UNSUPPORTED),
]
PNG_LENGTH_ROWS = [
    (dict(o=(4, 4, 3, 9), n=63), LENGTH, length(64, 63)),
    (dict(o=(4, 4, 2, 7), n=64), LENGTH, length(48, 64)),
    (dict(o=(5, 3, 0, 7), n=0, data=None), LENGTH, length(15, 0)),
    (dict(o=(MAX, MAX, 3, 7), n=7), LENGTH, length(MAX * MAX * 4, 7)),
]


def with_options(fn):
    def call(o=(4, 4, 3, 7), **kw):
        oc = png_options(*o) if o is not None else None
        return fn(C.byref(oc) if oc is not None else None, **kw)
    return call


def test_png_prepare():
    L = _lib.load()
    n_out, lay, ad = C.c_size_t(SENTINEL), _lib.PngLayoutC(), C.c_uint32()

    @with_options
    def call(o, data=P, n=64, out=P, cap=4096, out_len=C.byref(n_out), layout=C.byref(lay), adler=C.byref(ad)):
        return L.pixo_hip_png_prepare(data, n, o, out, cap, out_len, layout, adler)

    run(PNG_OPTION_ROWS + PNG_LENGTH_ROWS + [
        (dict(o=(4, 4, 3, 9), data=None, out_len=None), COMPRESSION, STRATEGY),
        (dict(data=None, out_len=None), COMPRESSION, null("data")),  # data before out_len
        (dict(out_len=None, layout=None), COMPRESSION, null("out_len")),
        (dict(layout=None, adler=None), COMPRESSION, null("layout")),
        (dict(adler=None, out=None, cap=0), COMPRESSION, null("adler32")),
    ], call)
    assert n_out.value == SENTINEL


def test_png_prepare_device():
    L = _lib.load()
    n_out, lay, ad = C.c_size_t(SENTINEL), _lib.PngLayoutC(), C.c_uint32()

    @with_options
    def call(o, n=None, px=P, out=P, layout=C.byref(lay), out_len=C.byref(n_out), adler=C.byref(ad)):
        return L.pixo_hip_png_prepare_device(px, o, out, layout, out_len, adler)

    run(PNG_OPTION_ROWS + [
        (dict(o=(4, 4, 3, 9), px=None), COMPRESSION, STRATEGY),
        (dict(px=None, out=None), COMPRESSION, null("d_pixels")),
        (dict(out=None, layout=None), COMPRESSION, null("d_out")),
        (dict(layout=None, out_len=None), COMPRESSION, null("layout")),  # layout before out_len here
        (dict(out_len=None, adler=None), COMPRESSION, null("out_len")),
        (dict(adler=None), COMPRESSION, null("adler32")),
    ], call)
    assert n_out.value == SENTINEL


def test_png_encode():
    L = _lib.load()
    p, n_out = C.POINTER(C.c_uint8)(), C.c_size_t(SENTINEL)

    @with_options
    def call(o, data=P, n=64, out=C.byref(p), out_len=C.byref(n_out)):
        return L.pixo_hip_png_encode(data, n, o, out, out_len)

    run(PNG_OPTION_ROWS + PNG_LENGTH_ROWS + [
        (dict(o=(4, 4, 3, 9), data=None), COMPRESSION, STRATEGY),
        (dict(data=None, out=None), COMPRESSION, null("data")),
        (dict(out=None, out_len=None), COMPRESSION, null("out")),
        (dict(out_len=None), COMPRESSION, null("out_len")),
    ], call)
    assert not p and n_out.value == SENTINEL


def test_png_encode_device():
    L = _lib.load()
    p, n_out = C.POINTER(C.c_uint8)(), C.c_size_t(SENTINEL)

    @with_options
    def call(o, n=None, px=P, out=C.byref(p), out_len=C.byref(n_out)):
        return L.pixo_hip_png_encode_device(px, o, out, out_len)

    run(PNG_OPTION_ROWS + [
        (dict(o=(4, 4, 3, 9), px=None), COMPRESSION, STRATEGY),
        (dict(px=None, out=None), COMPRESSION, null("d_pixels")),
        (dict(out=None, out_len=None), COMPRESSION, null("out")),
        (dict(out_len=None), COMPRESSION, null("out_len")),
    ], call)
    assert not p and n_out.value == SENTINEL


# ---- the row filters: png_plan's own order (dimensions, bpp, strategy), then data length, capacity, nulls ------------
PLAN_ROWS = [
    (dict(w=0, bpp=5, strategy=9), DIMS, dims(0, 4)),
    (dict(h=0, bpp=7), DIMS, dims(4, 0)),
    (dict(bpp=5, strategy=9), COLOUR, UNSUPPORTED),
    (dict(bpp=0), COLOUR, UNSUPPORTED),
    (dict(bpp=7), COLOUR, UNSUPPORTED),
    (dict(bpp=9), COLOUR, UNSUPPORTED),
    (dict(strategy=9), COMPRESSION, STRATEGY),
    (dict(w=MAX + 1, h=MAX + 1, strategy=255), COMPRESSION, STRATEGY),  # no upper limit of its own
]


def test_png_filter():
    L = _lib.load()
    out, ad = np.full(128, 0x5A, np.uint8), C.c_uint32(SENTINEL)

    def call(data=P, n=64, w=4, h=4, bpp=4, strategy=6, out=out.ctypes.data, cap=68, adler=C.byref(ad)):
        return L.pixo_hip_png_filter(data, n, w, h, bpp, strategy, 0, out, cap, adler)

    routes()
    run(PLAN_ROWS + [
        (dict(strategy=9, n=1, cap=0), COMPRESSION, STRATEGY),
        (dict(n=63, cap=0, data=None), LENGTH, length(64, 63)),
        (dict(bpp=6, n=64, cap=0), LENGTH, length(96, 64)),
        (dict(w=MAX, h=MAX, bpp=8, n=3), LENGTH, length(MAX * MAX * 8, 3)),
    ], call)
    assert routes() & CALLER_RETRY == 0
    # too small: inside the caller-storage scope only with storage AND a capacity; before the nulls, whose message names none
    for kw, retry in ((dict(cap=67, data=None), True), (dict(cap=1, adler=None), True), (dict(cap=0), False),
                      (dict(out=None, cap=67), False), (dict(out=None, cap=0, data=None, adler=None), False)):
        run([(kw, SMALL, small(68))], call)
        assert bool(routes() & CALLER_RETRY) == retry, kw
    run([
        (dict(data=None), COMPRESSION, "Compression error: null argument"),
        (dict(out=None, cap=68), COMPRESSION, "Compression error: null argument"),
        (dict(adler=None, cap=4096), COMPRESSION, "Compression error: null argument"),
    ], call)
    assert routes() == 0
    assert (out == 0x5A).all() and ad.value == SENTINEL  # a refusal writes nothing, the size needed is in the message only


def test_png_filter_device_and_async():
    L = _lib.load()
    ad = C.c_uint32(SENTINEL)

    def device(px=P, w=4, h=4, bpp=4, strategy=6, out=P, adler=C.byref(ad)):
        return L.pixo_hip_png_filter_device(px, w, h, bpp, strategy, 0, out, adler)

    def enqueue(w=4, h=4, bpp=4, strategy=6):
        return L.pixo_hip_png_filter_async(None, w, h, bpp, strategy, 0, None, None, None, None)

    run(PLAN_ROWS, enqueue)
    run(PLAN_ROWS + [
        (dict(strategy=9, px=None), COMPRESSION, STRATEGY),
        (dict(px=None, out=None), COMPRESSION, null("d_data")),
        (dict(out=None, adler=None), COMPRESSION, null("d_out")),
        (dict(adler=None), COMPRESSION, null("adler32")),
    ], device)
    assert ad.value == SENTINEL


# ---- zlib ---------------------------------------------------------------------------------------------------------------
def test_zlib_compress():
    L = _lib.load()
    p, n_out = C.POINTER(C.c_uint8)(), C.c_size_t(SENTINEL)

    def call(data=P, n=100, level=6, out=C.byref(p), out_len=C.byref(n_out)):
        return L.pixo_hip_zlib_compress(data, n, level, 4, 17, out, out_len)

    run([
        (dict(out=None, out_len=None, data=None), COMPRESSION, null("out")),
        (dict(out=None, n=0), COMPRESSION, null("out")),  # before the empty stream
        (dict(out_len=None, data=None), COMPRESSION, null("out_len")),
        (dict(out_len=None, n=0), COMPRESSION, null("out_len")),
        (dict(data=None), COMPRESSION, null("data")),
    ], call)
    assert not p and n_out.value == SENTINEL
    # no input: header, an empty fixed block, the Adler-32 of nothing — without a device, with or without a pointer
    for level, flg in ((0, 0x5E), (1, 0x5E), (2, 0x5E), (3, 0x9C), (6, 0x9C), (7, 0xDA), (9, 0xDA), (255, 0xDA)):
        for data in (None, P):
            assert call(data=data, n=0, level=level) == OK
            try:
                assert n_out.value == 8 and C.string_at(p, 8) == bytes([0x78, flg, 3, 0, 0, 0, 0, 1]), level
            finally:
                L.pixo_hip_free(p)


def test_zlib_compress_device():
    L = _lib.load()
    n_out = C.c_size_t(SENTINEL)

    def call(data=P, n=100000, out=P, cap=100016, out_len=C.byref(n_out)):
        return L.pixo_hip_zlib_compress_device(data, n, 6, 4, 17, out, cap, out_len)

    routes()
    run([
        (dict(out=None, out_len=None, cap=0), COMPRESSION, null("d_out")),
        (dict(out_len=None, cap=0, data=None), COMPRESSION, null("out_len")),
    ], call)
    assert n_out.value == SENTINEL
    # capacity before anything about d_data; the size comes back with the refusal; no caller-storage scope
    for kw, need in ((dict(cap=100015, data=None), 100016), (dict(cap=0), 100016), (dict(n=0, cap=7, data=None), 8),
                     (dict(n=1, cap=11), 12), (dict(n=65535, cap=0), 65546), (dict(n=65536, cap=0), 65552)):
        n_out.value = SENTINEL
        run([(kw, SMALL, small(need))], call)
        assert n_out.value == need, kw
    assert routes() == 0


# ---- resize --------------------------------------------------------------------------------------------------------------
# (`o`: pixo_resize_options as a tuple src w, src h, dst w, dst h, colour type, algorithm; None: a null options pointer)
RESIZE_PLAN_ROWS = [
    (dict(o=None), COMPRESSION, null("o")),
    (dict(o=(0, 4, 0, MAX + 1, 9, 9)), DIMS, dims(0, 4)),  # source before destination
    (dict(o=(4, 0, 2, 2, 3, 2)), DIMS, dims(4, 0)),
    (dict(o=(MAX + 1, 4, 2, 0, 9, 9)), DIMS, dims(2, 0)),  # destination before too large
    (dict(o=(4, 4, 0, 2, 3, 2)), DIMS, dims(0, 2)),
    (dict(o=(MAX + 1, 4, 2, 5, 9, 9)), LARGE, large(MAX + 1, 5)),  # the larger of each axis
    (dict(o=(4, MAX + 1, 2, 2, 3, 2)), LARGE, large(4, MAX + 1)),
    (dict(o=(4, 4, MAX + 1, 2, 3, 2)), LARGE, large(MAX + 1, 4)),
    (dict(o=(4, 3, 2, MAX + 2, 3, 2)), LARGE, large(4, MAX + 2)),
    (dict(o=(4, 4, 2, 2, 4, 3)), COLOUR_ARG, BAD_COLOUR % 4),  # colour type before algorithm
    (dict(o=(4, 4, 2, 2, 3, 3)), COLOUR_ARG, BAD_ALGORITHM % 3),
    (dict(o=(4, 4, 2, 2, 0, 255)), COLOUR_ARG, BAD_ALGORITHM % 255),
]
RESIZE_LENGTH_ROWS = [
    (dict(o=(4, 4, 2, 2, 3, 2), n=63, data=None), LENGTH, length(64, 63)),
    (dict(o=(4, 4, 2, 2, 0, 0), n=64), LENGTH, length(16, 64)),
    (dict(o=(5, 3, 2, 2, 1, 1), n=0), LENGTH, length(30, 0)),
    (dict(o=(MAX, MAX, 1, 1, 3, 2), n=1), LENGTH, length(MAX * MAX * 4, 1)),
]


def with_resize_options(fn):
    def call(o=(4, 4, 2, 2, 3, 2), **kw):
        oc = resize_options(*o) if o is not None else None
        return fn(C.byref(oc) if oc is not None else None, **kw)
    return call


def test_resize_into():
    L = _lib.load()
    n_out = C.c_size_t(SENTINEL)

    @with_resize_options
    def call(o, output=P, cap=16, data=P, n=64, out_len=C.byref(n_out)):
        return L.pixo_hip_resize_into(output, cap, data, n, o, out_len)

    routes()
    run([(dict(out_len=None, o=None), COMPRESSION, null("out_len")),  # out_len first
         (dict(out_len=None, o=(0, 0, 0, 0, 9, 9), cap=0, data=None, output=None), COMPRESSION, null("out_len"))]
        + [(dict(kw, cap=0), s, m) for kw, s, m in RESIZE_PLAN_ROWS + RESIZE_LENGTH_ROWS], call)
    assert n_out.value == SENTINEL and routes() == 0  # nothing is promised before the options hold
    # the size with the refusal; inside a caller-storage scope whatever the arguments; data and output only after it
    for kw, need in ((dict(cap=15), 16), (dict(cap=0, data=None), 16), (dict(cap=15, output=None, data=None), 16),
                     (dict(o=(4, 4, 7, 9, 2, 0), n=48, cap=188, output=None), 189)):
        n_out.value = SENTINEL
        run([(kw, SMALL, small(need))], call)
        assert n_out.value == need and routes() == CALLER_RETRY, kw
    n_out.value = SENTINEL
    run([(dict(data=None, output=None), COMPRESSION, null("data")),
         (dict(output=None, cap=4096), COMPRESSION, null("output"))], call)
    assert n_out.value == 16 and routes() == 0  # (written before the capacity was looked at)


def test_resize():
    L = _lib.load()
    p, n_out = C.POINTER(C.c_uint8)(), C.c_size_t(SENTINEL)

    @with_resize_options
    def call(o, data=P, n=64, out=C.byref(p), out_len=C.byref(n_out)):
        return L.pixo_hip_resize(data, n, o, out, out_len)

    run([(dict(out=None, out_len=None, o=None), COMPRESSION, null("out")),  # out and out_len before the options
         (dict(out_len=None, o=None), COMPRESSION, null("out_len"))]
        + RESIZE_PLAN_ROWS + RESIZE_LENGTH_ROWS
        + [(dict(data=None), COMPRESSION, null("data"))], call)
    assert not p and n_out.value == SENTINEL


def test_resize_image():
    L = _lib.load()
    p, n_out = C.POINTER(C.c_uint8)(), C.c_size_t(SENTINEL)

    def call(data=P, n=64, o=(4, 4, 2, 2, 3, 2), out=C.byref(p), out_len=C.byref(n_out)):
        return L.pixo_hip_resize_image(data, n, *o, out, out_len)

    run([  # wasm.rs:183-201: the two conversions first, before the pointers and before the dimensions
        (dict(o=(0, 0, 0, 0, 4, 3), out=None), COLOUR_ARG, BAD_COLOUR % 4),
        (dict(o=(0, 0, 0, 0, 3, 3), out=None), COLOUR_ARG, BAD_ALGORITHM % 3),
        (dict(o=(0, 4, 2, 2, 3, 2), out=None, out_len=None), COMPRESSION, null("out")),
        (dict(o=(0, 4, 2, 2, 3, 2), out_len=None), COMPRESSION, null("out_len")),
    ] + [(dict(o=kw["o"][:4] + (3, 2)), s, m) for kw, s, m in RESIZE_PLAN_ROWS if s in (DIMS, LARGE)] + RESIZE_LENGTH_ROWS
        + [(dict(data=None), COMPRESSION, null("data"))], call)
    assert not p and n_out.value == SENTINEL


def test_resize_device():
    L = _lib.load()

    @with_resize_options
    def call(o, n=None, data=None, src=P, dst=P):
        return L.pixo_hip_resize_device(src, o, dst, None)

    run(RESIZE_PLAN_ROWS + [
        (dict(o=(4, 4, 2, 2, 3, 3), src=None), COLOUR_ARG, BAD_ALGORITHM % 3),
        (dict(src=None, dst=None), COMPRESSION, null("d_src")),
        (dict(dst=None), COMPRESSION, null("d_dst")),
    ], call)


def test_resize_contributions():
    L = _lib.load()
    starts, counts, weights = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(256, np.float32)
    total = C.c_size_t(SENTINEL)

    def call(src=16, dst=8, s=starts.ctypes.data, c=counts.ctypes.data, w=weights.ctypes.data, cap=256, t=C.byref(total)):
        return L.pixo_hip_resize_contributions(src, dst, s, c, w, cap, t)

    routes()
    run([
        (dict(t=None, src=0), COMPRESSION, null("total")),
        (dict(src=0, dst=MAX + 1), DIMS, dims(0, MAX + 1)),
        (dict(src=MAX + 1, dst=0), DIMS, dims(MAX + 1, 0)),
        (dict(src=MAX + 1, dst=1, cap=0), LARGE, large(MAX + 1, 1)),
        (dict(src=1, dst=MAX + 1, s=None), LARGE, large(1, MAX + 1)),
    ], call)
    assert total.value == SENTINEL
    assert call() == OK and 8 < total.value <= 256
    need = total.value
    for kw in (dict(cap=need - 1), dict(cap=0, s=None, c=None, w=None)):  # its own wording: weights, not bytes
        total.value = SENTINEL
        run([(kw, SMALL, small(need, "weights"))], call)
        assert total.value == need
    assert routes() == 0  # (no caller-storage scope)
    run([(dict(s=None, c=None), COMPRESSION, null("starts")),
         (dict(c=None, w=None), COMPRESSION, null("counts")),
         (dict(w=None, cap=need), COMPRESSION, null("weights"))], call)
