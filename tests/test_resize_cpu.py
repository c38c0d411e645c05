"""Resize without a GPU: the C ABI's surface (symbols, struct, builder defaults), every error with its status, message and
order (the reference's own strings, recorded from its wasm build), the Lanczos3 contribution tables bit for bit against the
independent model, and the kernels' arithmetic (resize_math.h) compiled for the host over every golden vector."""
import ctypes as C

import numpy as np
import pytest

import emu_resize_lib as E
import resize_cases as RC
import resize_model as M
from pixo_amd import ColorType, _lib, error, resize

OK = RC.ok_cases()


def test_symbols_and_struct():
    L = _lib.load()
    for name in ("pixo_hip_resize", "pixo_hip_resize_into", "pixo_hip_resize_device", "pixo_hip_resize_image",
                 "pixo_hip_resize_contributions"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert C.sizeof(_lib.ResizeOptionsC) == 20  # 4 * u32 + 2 * u8 + pad
    assert _lib.ResizeOptionsC.color_type.offset == 16 and _lib.ResizeOptionsC.algorithm.offset == 17


def test_builder_defaults_follow_reference():
    o = resize.ResizeOptions.builder(30, 20).build()
    assert (o.src_width, o.src_height, o.dst_width, o.dst_height) == (30, 20, 30, 20)
    assert o.color_type == ColorType.Rgba and o.algorithm == resize.ResizeAlgorithm.Bilinear
    o = resize.ResizeOptions.builder(30, 20).dst(7, 9).color_type(ColorType.Gray).algorithm(resize.ResizeAlgorithm.Lanczos3).build()
    assert (o.dst_width, o.dst_height, o.color_type, o.algorithm) == (7, 9, 0, 2) and o.output_len() == 63
    assert [int(a) for a in resize.ResizeAlgorithm] == [0, 1, 2]
    assert resize.MAX_DIMENSION == 1 << 24


STATUS = {"Invalid image dimensions": (-1, error.InvalidDimensions), "Invalid pixel data length": (-2, error.InvalidDataLength),
          "Image ": (-4, error.ImageTooLarge), "Invalid color type": (-8, error.InvalidColorArgument),
          "Invalid resize algorithm": (-8, error.InvalidColorArgument)}


@pytest.mark.parametrize("c", RC.error_cases(), ids=lambda c: c["name"])
def test_errors_match_the_reference(c):
    """Checks fail before any work, so no GPU is needed; status, class and message, flat entry and struct entries."""
    status, cls = next(v for k, v in STATUS.items() if c["error"].startswith(k))
    px = RC.make_input(c)
    L = _lib.load()
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    rc = L.pixo_hip_resize_image(px.ctypes.data, px.size, c["sw"], c["sh"], c["dw"], c["dh"], c["color_type"], c["algorithm"],
                                 C.byref(out), C.byref(n))
    assert rc == status and L.pixo_hip_last_error().decode() == c["error"]
    with pytest.raises(cls) as e:
        resize.resize_image(px, c["sw"], c["sh"], c["dw"], c["dh"], c["color_type"], c["algorithm"])
    assert str(e.value) == c["error"]
    if c["color_type"] <= 3 and c["algorithm"] <= 2:
        o = resize.ResizeOptions(c["sw"], c["sh"], c["dw"], c["dh"], ColorType(c["color_type"]), resize.ResizeAlgorithm(c["algorithm"]))
        with pytest.raises(cls) as e:
            resize.resize(px, o)
        assert str(e.value) == c["error"]
        with pytest.raises(cls) as e:
            resize.resize_into(np.zeros(64, np.uint8), px, o)
        assert str(e.value) == c["error"]
        if status != -2:  # (a device pointer carries no length)
            oc = o._c()
            assert L.pixo_hip_resize_device(C.c_void_p(16), C.byref(oc), C.c_void_p(16), None) == status
            assert L.pixo_hip_last_error().decode() == c["error"]


def test_the_issue_strings_are_among_the_cases():
    msgs = {c["error"] for c in RC.error_cases()}
    for want in ("Invalid image dimensions: 0x48", "Invalid pixel data length: expected 9024 bytes, got 9216",
                 "Image 16777217x13 exceeds maximum dimension 16777216",
                 "Invalid color type: 9. Expected 0 (Gray), 1 (GrayAlpha), 2 (Rgb), or 3 (Rgba)",
                 "Invalid resize algorithm: 7. Expected 0 (Nearest), 1 (Bilinear), or 2 (Lanczos3)"):
        assert want in msgs


def test_resize_into_reports_the_length_before_any_work():
    o = resize.ResizeOptions.builder(8, 8).dst(4, 4).build()
    with pytest.raises(error.BufferTooSmall) as e:
        resize.resize_into(np.zeros(63, np.uint8), np.zeros(8 * 8 * 4, np.uint8), o)
    assert e.value.needed == 64


@pytest.mark.parametrize("src,dst", [(4096, 1024), (300, 2048), (64, 17), (7, 1), (1, 7), (1, 1), (31, 31), (1920, 640), (1080, 360),
                                     (997, 13), (13, 997), (2, 3), (100000, 3)])
def test_contributions_equal_the_model_bit_for_bit(src, dst):
    s, n, w = resize.contributions(src, dst)
    ms, mn, mw = M.contributions(src, dst)
    assert np.array_equal(s, ms) and np.array_equal(n, mn)
    assert w.size == mw.size
    d = np.flatnonzero(w.view(np.uint32) != mw.view(np.uint32))
    assert d.size == 0, "%d weights differ, first at %d: %r != %r" % (d.size, d[0], w[d[0]], mw[d[0]])


def test_contributions_capacity_and_size_query():
    L = _lib.load()
    total = C.c_size_t()
    assert L.pixo_hip_resize_contributions(64, 17, None, None, None, 0, C.byref(total)) == -9 and total.value == 378
    assert L.pixo_hip_resize_contributions(0, 17, None, None, None, 0, C.byref(total)) == -1
    # a 2^24 -> 1 down-scale: one destination index, every source index a tap
    assert L.pixo_hip_resize_contributions(1 << 24, 1, None, None, None, 0, C.byref(total)) == -9 and total.value == 1 << 24


def test_library_sinf_equals_the_models():
    x = np.concatenate([np.linspace(-9.43, 9.43, 40001), [0.0, 1e-5, -1e-5, 0.7853982, 2.3561945, 3.9269907, 5.4977875, 7.0685835]]).astype(np.float32)
    got = np.array([E.sinf(float(v)) for v in x], np.float32)
    assert np.array_equal(got.view(np.uint32), M.sinf(x).view(np.uint32))


@pytest.mark.parametrize("c", OK, ids=[c["name"] for c in OK])
def test_host_compiled_kernel_arithmetic_reproduces_golden(c):
    RC.check(c, E.resize(RC.make_input(c), c["sw"], c["sh"], c["dw"], c["dh"], RC.BPP[c["color_type"]], c["algorithm"]))
