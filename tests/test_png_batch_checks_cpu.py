"""CPU-only: the argument checks of the three PNG batch entries of the C ABI, in the order each entry runs them, in the
manner of test_entry_checks_cpu.py: one ordered table per entry, a row is a call with one defect, or with two so that the
ORDER of the two checks is pinned, and asserts the status and the exact pixo_hip_last_error() text.  Every check runs
before the thread's context is touched, so no row needs a device.
Order: the options (null, dimensions, too large, colour type, [host: data length = batch x one image], strategy), null
pixels, batch in 1..65535, the quantisation struct when one is given, null files / offsets, null lens."""
import ctypes as C

from pixo_amd import _lib
from test_entry_checks_cpu import BUF, COMPRESSION, LENGTH, MAX, P, PNG_OPTION_ROWS, STRATEGY, last_error, length, null, png_options, run, with_options

BATCH = "Compression error: batch must be 1..65535"


def quantization(mode=2, dithering=0, max_colors=16):
    return _lib.PngQuantizationC(mode, dithering, max_colors)


def bad_mode_text():
    """the text the single lossy entry gives for the same struct: the helper is shared, no new string"""
    L = _lib.load()
    o, q, p, n = png_options(), quantization(mode=9), C.POINTER(C.c_uint8)(), C.c_size_t()
    rc = L.pixo_hip_png_encode_lossy_device(P, C.byref(o), C.byref(q), C.byref(p), C.byref(n))
    assert rc != 0
    return rc, last_error()


def entry_rows(sink):
    """the rows every batch entry shares behind its options: `sink` names files or offsets"""
    q_rc, q_text = bad_mode_text()
    bad_q = quantization(mode=9)
    return [
        (dict(pixels=None, batch=0), COMPRESSION, null("pixels")),  # pixels before batch
        (dict(batch=0, q=C.byref(bad_q)), COMPRESSION, BATCH),  # batch before the quantisation
        (dict(batch=0), COMPRESSION, BATCH),
        (dict(batch=65536), COMPRESSION, BATCH),
        (dict(batch=65536, **{sink: None}), COMPRESSION, BATCH),
        (dict(q=C.byref(bad_q), **{sink: None}), q_rc, q_text),  # an unknown mode behind a valid options struct, before the sink
        (dict(q=C.byref(bad_q)), q_rc, q_text),
        (dict(**{sink: None}, lens=None), COMPRESSION, null(sink)),  # files / offsets before lens
        (dict(lens=None), COMPRESSION, null("lens")),
    ]


def test_png_encode_batch_device():
    L = _lib.load()
    files, lens = (C.POINTER(C.c_uint8) * 2)(), (C.c_size_t * 2)()

    @with_options
    def call(o, pixels=P, q=None, batch=2, files=files, lens=lens):
        return L.pixo_hip_png_encode_batch_device(pixels, o, q, batch, files, lens)

    run([r for r in PNG_OPTION_ROWS if "n" not in r[0]] + [
        (dict(o=(4, 4, 3, 9), pixels=None), COMPRESSION, STRATEGY),  # the options before pixels
    ] + entry_rows("files"), call)
    assert not files[0] and not files[1] and lens[0] == 0


def test_png_encode_batch_device_into():
    L = _lib.load()
    offsets, lens = (C.c_size_t * 2)(), (C.c_size_t * 2)()

    @with_options
    def call(o, pixels=P, q=None, batch=2, arena=P, cap=4096, offsets=offsets, lens=lens):
        return L.pixo_hip_png_encode_batch_device_into(pixels, o, q, batch, arena, cap, offsets, lens)

    run([r for r in PNG_OPTION_ROWS if "n" not in r[0]] + [
        (dict(o=(4, 4, 3, 9), pixels=None), COMPRESSION, STRATEGY),
        (dict(pixels=None, arena=None, cap=0), COMPRESSION, null("pixels")),  # a size query is checked like any call
    ] + entry_rows("offsets"), call)
    assert bytes(BUF) == bytes(4096), "a refused call wrote into the arena"


def test_png_encode_batch():
    L = _lib.load()
    files, lens = (C.POINTER(C.c_uint8) * 2)(), (C.c_size_t * 2)()

    bad_q = quantization(mode=9)

    @with_options
    def call(o, pixels=P, n=128, q=None, batch=2, files=files, lens=lens):
        return L.pixo_hip_png_encode_batch(pixels, n, o, q, batch, files, lens)

    run(PNG_OPTION_ROWS + [
        (dict(n=64), LENGTH, length(128, 64)),  # one image's length where the batch is two
        (dict(o=(4, 4, 3, 9), n=64), LENGTH, length(128, 64)),  # the length before the strategy
        (dict(n=127, pixels=None), LENGTH, length(128, 127)),  # ... and before pixels
        (dict(o=(4, 4, 2, 7), n=128), LENGTH, length(96, 128)),
        (dict(batch=0, n=128), LENGTH, length(0, 128)),  # batch x one image: nothing is the right length for no image
        (dict(batch=65536, n=128), LENGTH, length(65536 * 64, 128)),
        (dict(o=(MAX, MAX, 3, 7), batch=65535, n=7), LENGTH, length((1 << 64) - 1, 7)),  # the product does not fit: no length is right
        (dict(o=(4, 4, 3, 9), pixels=None), COMPRESSION, STRATEGY),
        (dict(batch=0, n=0), COMPRESSION, BATCH),
        (dict(batch=65536, n=65536 * 64), COMPRESSION, BATCH),
        (dict(pixels=None, batch=0, n=0), COMPRESSION, null("pixels")),  # pixels before batch
        (dict(batch=0, n=0, q=C.byref(bad_q)), COMPRESSION, BATCH),  # batch before the quantisation
    ] + [r for r in entry_rows("files") if r[0].get("batch", 2) == 2], call)
    assert not files[0] and not files[1] and lens[0] == 0
