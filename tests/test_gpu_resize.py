"""GPU parity of resize (pixo_hip_resize*, resize.hip) through the C ABI: every vector made by the reference's own wasm build
byte for byte through each entry point, seeded random cases against the independent model, the buffer life cycle, the
pipeline into the encoders.  A single differing byte fails; the message names the case and the first differing index.
No test here provokes a fault; nothing starts a child process.  -m gpu."""
import hashlib
import threading

import numpy as np
import pytest

import oracle_lib as O
import resize_cases as RC
import resize_model as M
from pixo_amd import ColorType, error, jpeg, png, resize

pytestmark = pytest.mark.gpu

OK = RC.ok_cases()
IDS = [c["name"] for c in OK]
_torch = None


def torch():
    global _torch
    if _torch is None:
        import torch as t
        _torch = t
    return _torch


def options(c):
    return resize.ResizeOptions.builder(c["sw"], c["sh"]).dst(c["dw"], c["dh"]).color_type(ColorType(c["color_type"])) \
        .algorithm(resize.ResizeAlgorithm(c["algorithm"])).build()


def on_device(px, offset=0):
    t = torch()
    buf = t.zeros(px.size + offset + 16, dtype=t.uint8, device="cuda:0")
    buf[offset:offset + px.size] = t.from_numpy(np.ascontiguousarray(px)).to("cuda:0")
    return buf[offset:offset + px.size]


def device_resize(c, px, stream=0, src_offset=0, dst_offset=0):
    t = torch()
    o = options(c)
    d_src = on_device(px, src_offset)
    d_all = t.full((o.output_len() + dst_offset + 16,), 0xA5, dtype=t.uint8, device="cuda:0")
    d_dst = d_all[dst_offset:dst_offset + o.output_len()]
    t.cuda.synchronize()
    resize.resize_device(d_src, o, d_dst, stream)
    t.cuda.synchronize()
    got = d_all.cpu().numpy()
    assert (got[:dst_offset] == 0xA5).all() and (got[dst_offset + o.output_len():] == 0xA5).all(), "%s: bytes outside the output were written" % c["name"]
    return got[dst_offset:dst_offset + o.output_len()].tobytes()


@pytest.mark.parametrize("c", OK, ids=IDS)
def test_golden_resize(c):
    RC.check(c, resize.resize(RC.make_input(c), options(c)))


@pytest.mark.parametrize("c", OK, ids=IDS)
def test_golden_resize_into(c):
    out = np.full(c["len"] + 32, 0x5A, np.uint8)
    n = resize.resize_into(out, RC.make_input(c), options(c))
    assert n == c["len"] and (out[n:] == 0x5A).all()
    RC.check(c, out[:n].tobytes())


@pytest.mark.parametrize("c", OK, ids=IDS)
def test_golden_resize_image(c):
    RC.check(c, resize.resize_image(RC.make_input(c), c["sw"], c["sh"], c["dw"], c["dh"], c["color_type"], c["algorithm"]))


@pytest.mark.parametrize("c", OK, ids=IDS)
def test_golden_resize_device(c):
    RC.check(c, device_resize(c, RC.make_input(c)))


@pytest.mark.parametrize("c", [c for c in OK if c["len"] <= 12000][::5], ids=lambda c: c["name"])
def test_golden_resize_device_unaligned_pointers(c):
    """Source and destination 1-3 bytes off a dword: the kernels' dword paths must give way to bytes."""
    px = RC.make_input(c)
    for so, do in ((1, 3), (2, 1), (3, 2)):
        RC.check(c, device_resize(c, px, src_offset=so, dst_offset=do))


def test_random_cases_against_the_model():
    bad = []
    for i, c in enumerate(RC.random_cases(20261, 200)):
        px = RC.make_input(c)
        want = M.resize(px, c["sw"], c["sh"], c["dw"], c["dh"], RC.BPP[c["color_type"]], c["algorithm"])
        got = resize.resize(px, options(c)) if i % 2 else device_resize(c, px)
        diff = RC.first_difference(got, want)
        if diff:
            bad.append("%s: %s" % (c["name"], diff))
    assert not bad, "\n".join(bad[:20])


def test_resize_into_short_buffer():
    c = next(c for c in OK if c["name"].startswith("lanczos3_64x48_to_17x13_c2"))
    out = np.zeros(c["len"] - 1, np.uint8)
    with pytest.raises(error.BufferTooSmall) as e:
        resize.resize_into(out, RC.make_input(c), options(c))
    assert e.value.needed == c["len"]
    assert (out == 0).all()
    out = np.zeros(c["len"], np.uint8)
    assert resize.resize_into(out, RC.make_input(c), options(c)) == c["len"]
    RC.check(c, out.tobytes())


def _by_prefix(prefix):
    return next(c for c in OK if c["name"].startswith(prefix))


def test_grow_pair_and_trim_in_one_context():
    """small, large, small in one context (the buffers grow, the tables change and come back), a trim between calls."""
    import ctypes as C
    from pixo_amd import _lib
    small, large = _by_prefix("lanczos3_64x48_to_17x13_c3"), _by_prefix("lanczos3_1920x1080_to_640x360_c3")
    for c in (small, large, small, small):
        RC.check(c, resize.resize(RC.make_input(c), options(c)))
    assert _lib.load().pixo_hip_trim() == 0
    for c in (small, large):
        RC.check(c, resize.resize(RC.make_input(c), options(c)))
        RC.check(c, device_resize(c, RC.make_input(c)))
    assert _lib.load().pixo_hip_trim() == 0
    RC.check(small, device_resize(small, RC.make_input(small)))


def test_route_bits_are_seen():
    for algo, bit in ((0, resize.ROUTE_RESIZE_NEAREST), (1, resize.ROUTE_RESIZE_BILINEAR), (2, resize.ROUTE_RESIZE_LANCZOS3)):
        c = _by_prefix("%s_37x23_to_64x41_c2" % RC.ALGO_NAMES[algo])
        jpeg.debug_routes(clear=True)
        RC.check(c, resize.resize(RC.make_input(c), options(c)))
        bits = jpeg.debug_routes(clear=True)
        assert bits & (resize.ROUTE_RESIZE_NEAREST | resize.ROUTE_RESIZE_BILINEAR | resize.ROUTE_RESIZE_LANCZOS3) == bit


@pytest.mark.parametrize("prefix", ["lanczos3_160x120_to_61x47_c2_photo", "bilinear_1920x1080_to_640x360_c2_photo",
                                    "lanczos3_1920x1080_to_640x360_c2_photo"])
def test_pipeline_resize_then_jpeg_on_one_stream(prefix):
    """resize_device -> jpeg.encode_device on the same stream, no host synchronisation between them, equals the oracle's
    file of the (model-checked) resized pixels."""
    t = torch()
    c = _by_prefix(prefix)
    px = RC.make_input(c)
    want_px = np.frombuffer(M.resize(px, c["sw"], c["sh"], c["dw"], c["dh"], 3, c["algorithm"]), np.uint8)
    RC.check(c, want_px.tobytes())
    s = t.cuda.Stream()
    with t.cuda.stream(s):
        d_src = t.from_numpy(px).to("cuda:0", non_blocking=False)
        d_dst = t.empty(c["len"], dtype=t.uint8, device="cuda:0")
    with jpeg.producer_stream(s.cuda_stream):
        resize.resize_device(d_src, options(c), d_dst, s.cuda_stream)
        jo = jpeg.JpegOptions.builder(c["dw"], c["dh"]).color_type(ColorType.Rgb).quality(80).subsampling(jpeg.Subsampling.S420).build()
        got = jpeg.encode_device(d_dst, jo)
    t.cuda.synchronize()
    assert got == O.encode(want_px, O.make_options(c["dw"], c["dh"], O.RGB, 80, O.S420)), c["name"]


def test_pipeline_resize_then_png_filters_on_one_stream():
    t = torch()
    c = _by_prefix("lanczos3_1920x1080_to_640x360_c3")
    px = RC.make_input(c)
    want_px = np.frombuffer(M.resize(px, c["sw"], c["sh"], c["dw"], c["dh"], 4, c["algorithm"]), np.uint8)
    RC.check(c, want_px.tobytes())
    s = t.cuda.Stream()
    with t.cuda.stream(s):
        d_src = t.from_numpy(px).to("cuda:0")
        d_dst = t.empty(c["len"], dtype=t.uint8, device="cuda:0")
        d_flt = t.empty(png.filtered_size(c["dw"], c["dh"], 4), dtype=t.uint8, device="cuda:0")
    with jpeg.producer_stream(s.cuda_stream):
        resize.resize_device(d_src, options(c), d_dst, s.cuda_stream)
        adler = png.apply_filters_device(d_dst, c["dw"], c["dh"], 4, d_flt, png.FilterStrategy.ADAPTIVE)
    t.cuda.synchronize()
    oflt, oadler = O.png_filter(want_px, c["dw"], c["dh"], 4, O.S_ADAPTIVE)
    assert adler == oadler and np.array_equal(d_flt.cpu().numpy(), oflt)


def test_two_calling_threads():
    cases = [c for c in OK if c["len"] <= 12000]
    errors = []

    def work(k):
        try:
            for rep in range(2):
                for c in cases[k::2]:
                    RC.check(c, resize.resize(RC.make_input(c), options(c)))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert not any(th.is_alive() for th in threads), "a calling thread did not finish"
    assert not errors, errors[:3]


@pytest.mark.parametrize("c", RC.error_cases(), ids=lambda c: c["name"])
def test_errors_on_the_gpu_machine_too(c):
    with pytest.raises(error.Error) as e:
        resize.resize_image(RC.make_input(c), c["sw"], c["sh"], c["dw"], c["dh"], c["color_type"], c["algorithm"])
    assert str(e.value) == c["error"]
