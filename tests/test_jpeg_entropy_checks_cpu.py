"""PIXO_DECODE_DEVICE_ENTROPY without a GPU: the flag's bit, the keyword on the Python entries, what the plan sends to the
device, the geometry entry, and the checks that come before anything touches a device."""
import inspect

import pytest

import jpeg_decode_cases as JC
import jpeg_entropy_cases as EC
import png_decode_cases as PC


def D():
    from pixo_amd import decode
    return decode


def test_the_keyword_and_the_bits_exist():
    d = D()
    assert d.DEVICE_ENTROPY == 4 and d._flags(True, True, True) == 7
    for f in (d.decode_jpeg_batch, d.decode_jpeg_batch_device, d.decode_jpeg_batch_plan, d.decode_jpeg_batch_timed):
        assert inspect.signature(f).parameters["device_entropy"].default is False, f.__name__
    assert d.ROUTE_JPEG_ENTROPY_DEVICE == 1 << 50 and d.ROUTE_JPEG_ENTROPY_HOST_REDO == 1 << 51


def test_geometry_is_consistent():
    g = D().decode_jpeg_entropy_geometry()
    e = EC.geometry()
    assert g == {k: e[k] for k in g}  # the library's is the emulation's
    assert g["sub_bytes"] >= 32 and g["sub_bytes"] % 16 == 0 and g["group_subs"] % 64 == 0
    assert g["sub_bytes"] * g["group_subs"] <= 64 * 1024  # a workgroup's span fits LDS
    assert 1 <= g["min_scan_bytes"] <= g["sub_bytes"] and g["round_cap"] >= 1
    from pixo_amd import _lib
    _lib.load().pixo_hip_jpeg_entropy_geometry(None, None, None, None)  # any pointer may be null


def test_plan_sends_restart_files_short_scans_and_empty_images_to_the_host():
    d = D()
    names = ["420_50x37_q80", "422_50x37_q80_rst5", "gray_1x1_q80", "444_50x37_q80", "gray_50x37_q80"]
    files = [JC.data(JC.by_name(n)) for n in names]
    assert b"\xff\xdd" in files[1] and len(EC.scan_of(files[2])) < d.decode_jpeg_entropy_geometry()["min_scan_bytes"]
    off = d.decode_jpeg_batch_plan(files)
    on = d.decode_jpeg_batch_plan(files, device_entropy=True)
    assert off["on_device"] == [False] * 5 and on["on_device"] == [True, False, False, True, True]
    for k in ("classes", "launches", "threads", "sub_first"):
        assert on[k] == off[k]


def test_sub_batches_count_the_scans_under_the_flag():
    """A limit that holds two files' coefficients and not two files' coefficients with their records and scans"""
    from pixo_amd import jpeg
    d = D()
    one = EC.borders()["three_workgroups"]  # 640 x 480, 4:2:0: 921,600 bytes of coefficients, a scan of some 316,000
    coef = 640 * 480 * 3
    assert coef // 8 < len(EC.scan_of(one))
    files = [one] * 3
    jpeg.debug_configure("decode_batch_bytes=%d" % (2 * coef + coef // 8))
    try:
        off = d.decode_jpeg_batch_plan(files)
        on = d.decode_jpeg_batch_plan(files, device_entropy=True)
    finally:
        jpeg.debug_configure("")
    assert off["sub_first"] == [0, 2, 3] and on["sub_first"] == [0, 1, 2, 3] and on["on_device"] == [True] * 3


def test_phase_one_refusals_are_the_same_with_the_flag():
    from pixo_amd import error
    d = D()
    good = JC.data(JC.by_name("420_17x17_q80"))
    for bad, words in ((b"nothing", "not a JPEG file"), (good[:2] + b"\xff\xc2\x00\x02" + good[2:], "progressive JPEG not supported")):
        for entry in (d.decode_jpeg_batch, d.decode_jpeg_batch_plan):
            with pytest.raises(error.Error) as a:
                entry([good, bad], device_entropy=True)
            with pytest.raises(error.Error) as b:
                entry([good, bad])
            assert str(a.value) == str(b.value) and words in str(a.value) and str(a.value).endswith("(image 1)")


def test_png_entries_ignore_the_flag():
    """The PNG plan under flags 4 is the plan under flags 0 (the JPEG entries ignore the inflate flag in the same way)"""
    import ctypes as C
    from pixo_amd import _lib
    d = D()
    L = _lib.load()
    files = [PC.make(33, 17, PC.RGB, 8, seed=1), PC.make(9, 9, PC.GRAY, 8, seed=2)]
    arr, held = d._files_c(files)

    def plan(flags):
        sub_first, runs = (C.c_uint32 * 3)(), (C.c_uint64 * 2)()
        subs, unfilter, convert, threads = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _lib.check(L.pixo_hip_debug_png_decode_batch_plan(arr, 2, flags, sub_first, C.byref(subs), runs, C.byref(unfilter), C.byref(convert), C.byref(threads)))
        return list(sub_first), list(runs), subs.value, unfilter.value, convert.value, threads.value
    assert plan(d.DEVICE_ENTROPY) == plan(0) and plan(d.DEVICE_ENTROPY | d.ONE_THREAD) == plan(d.ONE_THREAD)
    # ... and the JPEG plan under the inflate flag is the plan without it
    one = [JC.data(JC.by_name("420_50x37_q80"))]
    arr, held = d._files_c(one)

    def jpeg_on_device(flags):
        on, sub_first, subs = (C.c_uint8 * 1)(), (C.c_uint32 * 2)(), C.c_uint32()
        _lib.check(L.pixo_hip_debug_jpeg_entropy_plan(arr, 1, flags, on, sub_first, C.byref(subs)))
        return on[0]
    assert [jpeg_on_device(f) for f in (0, d.DEVICE_INFLATE, d.DEVICE_ENTROPY, d.DEVICE_ENTROPY | d.DEVICE_INFLATE)] == [0, 0, 1, 1]
