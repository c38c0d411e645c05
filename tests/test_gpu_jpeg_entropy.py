"""PIXO_DECODE_DEVICE_ENTROPY on the device (jpeg_entropy_dec.hip): with the flag image i is byte for byte what the entry
returns without it, a refused batch is refused with the same status and words, and the coefficients the device vouches for are
the host decoder's — over the committed decode cases, the border files of tests/jpeg_entropy_cases.py (placed by
pixo_hip_jpeg_entropy_geometry), a scan that never synchronises, refusals and mixtures, sub-batches and growing buffers.  Every
file is tiny.  The malformed files are inputs the entry must survive; the host emulation ran them first
(test_emu_jpeg_entropy_dec.py)."""
import numpy as np
import pytest

import jpeg_decode_cases as JC
import jpeg_entropy_cases as EC

pytestmark = pytest.mark.gpu


def D():
    from pixo_amd import decode
    return decode


def routes_of(call):
    """(what call() returns or the Error it raises, the route bits it set)"""
    from pixo_amd import error, jpeg
    jpeg.debug_routes(clear=True)
    try:
        got = call()
    except error.Error as e:
        got = e
    return got, jpeg.debug_routes(clear=True)


def outcome(files, **kw):
    """The images' (width, height, colour type, pixels), or the refusal's (status class, words)"""
    from pixo_amd import error
    try:
        return [(im.width, im.height, int(im.color_type), im.pixels) for im in D().decode_jpeg_batch(files, **kw)]
    except error.Error as e:
        return type(e).__name__, str(e)


def host_coefficients(data, component):
    return D().decode_jpeg_coefficients(data, component)


def assert_device_coefficients_are_the_hosts(files, vouched):
    d = D()
    for component in range(3):
        res = d.decode_jpeg_entropy_debug(files, component)
        for i, (f, r) in enumerate(zip(files, res)):
            assert r["vouched"] == vouched[i], (i, r["why"], r["rounds"])
            if r["coef"] is not None:
                assert np.array_equal(r["coef"], host_coefficients(f, component)), (i, component)


CLASSES = ("gray", "444", "422", "420")


@pytest.mark.parametrize("which", CLASSES + ("synth", "mixed"))
def test_committed_cases(which):
    d = D()
    cases = JC.SYNTH if which == "synth" else JC.CASES[::3] + JC.SYNTH[::4] if which == "mixed" else [c for c in JC.CASES if c["name"].startswith(which)]
    files = [JC.data(c) for c in cases]
    emu = [EC.emulate(f) for f in files]
    images, bits = routes_of(lambda: d.decode_jpeg_batch(files, device_entropy=True))
    plain = d.decode_jpeg_batch(files)
    for c, im, p in zip(cases, images, plain):
        assert im == p and JC.mismatch(im.pixels, c) == ""
    assert bits & d.ROUTE_JPEG_ENTROPY_DEVICE
    if all(e["vouched"] for e in emu if e["status"] == 0):
        assert not bits & d.ROUTE_JPEG_ENTROPY_HOST_REDO
    plan = d.decode_jpeg_batch_plan(files, device_entropy=True)
    assert plan["on_device"] == [e["status"] == 0 for e in emu]
    assert_device_coefficients_are_the_hosts(files, [e["vouched"] for e in emu])
    res = d.decode_jpeg_entropy_debug(files)
    for e, r in zip(emu, res):
        assert (r["why"], r["subs"]) == ((e["why"], e["subs"]) if e["status"] == 0 else (d.ENTROPY_HOST, 0))
        assert r["rounds"] == (e["rounds"] if e["status"] == 0 else 0)  # (one file a workgroup here: the emulation's count)


def test_the_library_geometry_is_the_emulations():
    g = D().decode_jpeg_entropy_geometry()
    assert g == {k: EC.geometry()[k] for k in g}


@pytest.mark.parametrize("name", sorted(EC.borders()))
def test_borders(name):
    d = D()
    f = EC.borders()[name]
    e = EC.emulate(f)
    assert e["vouched"]
    got, bits = routes_of(lambda: outcome([f], device_entropy=True))
    assert got == outcome([f]) and isinstance(got, list)
    assert bits & d.ROUTE_JPEG_ENTROPY_DEVICE and not bits & d.ROUTE_JPEG_ENTROPY_HOST_REDO
    res = d.decode_jpeg_entropy_debug([f])[0]
    assert res["vouched"] and res["subs"] == e["subs"]
    ncomp = 1 if name != "three_workgroups" and name != "sixteen_bit_codes" else 3
    for component in range(ncomp):
        assert np.array_equal(d.decode_jpeg_entropy_debug([f], component)[0]["coef"], host_coefficients(f, component))


def test_all_border_files_in_one_batch():
    files = list(EC.borders().values())
    got, bits = routes_of(lambda: outcome(files, device_entropy=True))
    assert got == outcome(files)
    assert not bits & D().ROUTE_JPEG_ENTROPY_HOST_REDO


def test_a_scan_that_never_synchronises():
    """Below the cap: vouched, the rounds the emulation counts (a round per subsequence), the cap not reached.  Above: the device
    does not vouch, the host decodes again, the pixels are right."""
    d = D()
    cap = d.decode_jpeg_entropy_geometry()["round_cap"]
    short, long = EC.never_synchronises(cap - 32), EC.never_synchronises(cap + 18)
    es, el = EC.emulate(short), EC.emulate(long)
    assert es["vouched"] and es["rounds"] == es["subs"] - 1 < cap and not el["vouched"] and el["rounds"] == cap
    rs, rl = d.decode_jpeg_entropy_debug([short, long])
    assert rs["vouched"] and rs["rounds"] == es["rounds"] and np.array_equal(rs["coef"], host_coefficients(short, 0))
    assert not rl["vouched"] and rl["why"] == d.ENTROPY_NOT_SETTLED and rl["rounds"] == cap
    got, bits = routes_of(lambda: outcome([short], device_entropy=True))
    assert got == outcome([short]) and not bits & d.ROUTE_JPEG_ENTROPY_HOST_REDO
    got, bits = routes_of(lambda: outcome([long, short], device_entropy=True))
    assert got == outcome([long, short]) and bits & d.ROUTE_JPEG_ENTROPY_HOST_REDO and bits & d.ROUTE_JPEG_ENTROPY_DEVICE
    assert set(got[0][3]) == {128}  # (all coefficients zero)
    # a smaller cap through the debug entry: the short file is not vouched for either
    assert d.decode_jpeg_entropy_debug([short], round_cap=7)[0]["why"] == d.ENTROPY_NOT_SETTLED


def mixture():
    names = ("gray_50x37_q80", "444_50x37_q80", "422_50x37_q80", "420_50x37_q80", "422_50x37_q80_rst5")
    files = [JC.data(JC.by_name(n)) for n in names]
    empty = JC.data(JC.by_name("gray_50x37_q80"))
    sof = empty.index(b"\xff\xc0")
    files.append(empty[:sof + 5] + b"\x00\x00" + empty[sof + 7:])  # (height zero: an image without MCUs)
    return files


def test_mixture_with_a_restart_file_an_empty_image_and_an_odd_address():
    import ctypes as C
    from pixo_amd import _lib
    d = D()
    files = mixture()
    want = outcome(files)
    assert isinstance(want, list) and want[5][:2] == (50, 0)
    assert outcome(files, device_entropy=True) == want and outcome(files, device_entropy=True, one_thread=True) == want
    # one file at an odd host address
    raw = np.zeros(len(files[3]) + 1, np.uint8)
    raw[1:] = np.frombuffer(files[3], np.uint8)
    assert raw[1:].ctypes.data % 2 == 1
    L = _lib.load()
    arr = (_lib.PngFileC * 2)(_lib.PngFileC(raw[1:].ctypes.data, len(files[3])), _lib.PngFileC(raw[1:].ctypes.data, len(files[3])))
    images, out, n = (_lib.PngImageC * 2)(), C.POINTER(C.c_uint8)(), C.c_size_t()
    _lib.check(L.pixo_hip_jpeg_decode_batch(arr, 2, d.DEVICE_ENTROPY, C.byref(out), C.byref(n), images))
    block = _lib.take(L, out, n)
    assert block[images[1].offset:images[1].offset + len(want[3][3])] == want[3][3] == block[:len(want[3][3])]
    # the device entry, into a tensor
    import torch
    views = d.decode_jpeg_batch_device(files, device_entropy=True)
    torch.cuda.synchronize()
    for (t, _), w in zip(views, want):
        assert t.cpu().numpy().tobytes() == w[3]


@pytest.mark.parametrize("name", sorted(EC.malformed()))
def test_refusals_are_the_host_paths(name):
    d = D()
    bad, words = EC.malformed()[name]
    good = JC.data(JC.by_name("420_50x37_q80"))
    for files in ([good, bad, good], [bad], [good, good, bad, bad]):
        want = outcome(files)
        got, bits = routes_of(lambda: outcome(files, device_entropy=True))
        assert got == want and isinstance(want, tuple), want
        assert want[1].endswith(" (image %d)" % files.index(bad)) and (words is None or words in want[1])
        assert bits & d.ROUTE_JPEG_ENTROPY_HOST_REDO
    assert not d.decode_jpeg_entropy_debug([bad])[0]["vouched"]


def test_two_bad_files_answer_with_the_lower_index():
    m = EC.malformed()
    good = JC.data(JC.by_name("444_50x37_q80"))
    files = [good, m["index_past_63"][0], good, m["cut_at_200"][0]]
    want = outcome(files)
    assert outcome(files, device_entropy=True) == want and "coefficient index past 63 (image 1)" in want[1]
    files = [good, m["cut_at_200"][0], m["index_past_63"][0]]
    want = outcome(files)
    assert outcome(files, device_entropy=True) == want and "entropy-coded segment ends early (image 1)" in want[1]
    # ... and a restart file the host refuses from the start in front of one the device does not vouch for
    rst = JC.data(JC.by_name("422_50x37_q80_rst5"))
    files = [good, rst[:-30], m["index_past_63"][0]]
    want = outcome(files)
    assert outcome(files, device_entropy=True) == want and want[1].endswith("(image 1)")


def test_fifty_single_byte_mutations_of_a_small_scan():
    """Each outcome, pixels or words, is the host path's"""
    base = EC.written("420", 48, 32, 71, density=0.3)
    head = len(base) - len(EC.scan_of(base))
    rng = np.random.default_rng(72)
    files = []
    for _ in range(50):
        v = bytearray(base)
        v[head + int(rng.integers(0, len(base) - head - 2))] = int(rng.integers(0, 256)) if rng.random() < 0.7 else 0xFF
        files.append(bytes(v))
    kinds = set()
    for f in files:
        want = outcome([f])
        assert outcome([f], device_entropy=True) == want
        kinds.add(type(want))
    assert kinds == {list, tuple}  # (some decode, some are refused)
    good = [f for f in files if isinstance(outcome([f]), list)]
    assert outcome(good, device_entropy=True) == outcome(good)


def test_two_sub_batches_and_two_calls_with_growing_buffers():
    from pixo_amd import jpeg
    d = D()
    cases = [c for c in JC.CASES if c["w"] == 50][:12]
    files = [JC.data(c) for c in cases]
    jpeg.debug_configure("decode_batch_bytes=65536")
    try:
        plan = d.decode_jpeg_batch_plan(files, device_entropy=True)
        got = outcome(files, device_entropy=True)
    finally:
        jpeg.debug_configure("")
    assert len(plan["sub_first"]) > 2 and got == outcome(files)
    for c, g in zip(cases, got):
        assert JC.mismatch(g[3], c) == ""
    # a small call, a larger one, the small one again: the context's buffers grow and are reused
    small, large = [files[0]], [EC.borders()["three_workgroups"], files[1]]
    a = outcome(small, device_entropy=True)
    b = outcome(large, device_entropy=True)
    assert a == outcome(small) and b == outcome(large) and outcome(small, device_entropy=True) == a


def test_timed_entry_and_last_call_record():
    d = D()
    files = [EC.borders()["ff00_straddles_a_border"], EC.never_synchronises(d.decode_jpeg_entropy_geometry()["round_cap"] + 18)]
    ms = d.decode_jpeg_batch_timed(files, device_entropy=True)
    last = d.decode_jpeg_entropy_last()
    assert len(ms) == 5 and all(x >= 0 for x in ms) and ms[4] >= ms[0]
    assert last["files_device"] == 2 and last["files_redone"] == 1 and last["rounds"] == d.decode_jpeg_entropy_geometry()["round_cap"] and last["device_ms"] > 0
