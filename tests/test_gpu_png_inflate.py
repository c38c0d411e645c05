"""Inflate on the device for the PNG decode batches (pixo_amd/csrc/png_inflate.hip; PIXO_DECODE_DEVICE_INFLATE): the kernel alone
over every case of tests/inflate_cases.py in one launch — bytes and Adler-32 against zlib, verdicts, the bytes it must not touch,
and every figure against the host build of the same walk —, then the batch entries with the flag against the same calls without
it: every shape and filter layout, split IDATs, the library's own encoder's files at both efforts, the stored whole-file vectors,
every refusal only the inflated streams show, the host's second inflate of an over-subscribed stream, sub-batches, odd caller
addresses and the thread flag."""
import struct
import zlib

import numpy as np
import pytest

import inflate_cases as IC
import png_decode_cases as PC
import png_decode_model as M
import png_file_cases as FC

pytestmark = pytest.mark.gpu

OK, FAILED, NEEDS_HOST = 0, 1, 2


def lib():
    from pixo_amd import decode
    return decode


def constants():
    d = lib()
    return d.inflate_step_tokens(), d.inflate_window_bytes(), d.inflate_far_distance(), d.inflate_stored_chunk()


CASES = [c for c in IC.cases(*constants()) if c["kind"] != "header"]
BIT_DEVICE, BIT_REDO = 1 << 43, 1 << 44


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------
def run_alone(cases, shift):
    """Every case in ONE launch: region i starts `shift` bytes behind a multiple of 16, 48 guard bytes lie between regions, the
    block is filled with 0xA5.  An empty stream at the block's end makes the entry carry the last guard too."""
    at, out_at = 64 + shift, []
    for c in cases:
        out_at.append(at)
        at = (at + c["expected"] + 48 + 15) // 16 * 16 + shift
    block = np.full(at + 64, 0xA5, np.uint8)
    streams = [c["z"] for c in cases] + [zlib.compress(b"")]
    expected = [c["expected"] for c in cases] + [0]
    verdicts, produced, adlers, ms = lib().inflate_zlib_batch_debug(streams, expected, block, out_at + [block.size])
    assert verdicts[-1] == OK and produced[-1] == 0 and adlers[-1] == 1 and ms > 0
    return block, out_at, verdicts, produced, adlers


@pytest.mark.parametrize("shift", (0, 5))
def test_every_case_in_one_launch(shift):
    import emu_png_inflate_lib as E
    block, out_at, verdicts, produced, adlers = run_alone(CASES, shift)
    written = np.zeros(block.size, bool)
    for c, at, v, n, a in zip(CASES, out_at, verdicts, produced, adlers):
        got = block[at:at + c["expected"]].tobytes()
        assert n <= c["expected"], c["name"]
        written[at:at + n] = True
        assert a == zlib.adler32(got[:n]), c["name"]  # the Adler-32 is that of the bytes produced, whatever the verdict
        if c["kind"] == "ok":
            assert (v, n) == (OK, c["expected"]) and got == c["data"], c["name"]
            assert a == zlib.adler32(c["data"]) == int.from_bytes(c["z"][-4:], "big"), c["name"]
        elif c["kind"] == "needs_host":
            assert (v, n) == (NEEDS_HOST, 0), c["name"]
        else:
            assert v == FAILED, c["name"]
        r = E.inflate(c["z"], c["expected"])  # the same walk, lane by lane on the host
        assert (v, n, a) == (r["verdict"], r["produced"], r["adler"]) and got == r["out"], c["name"]
    assert (block[~written] == 0xA5).all(), "a byte outside the produced bytes was written"


def test_many_streams_of_one_launch_do_not_disturb_each_other():
    """More streams than compute units, long and short mixed, each checked: nothing is shared between workgroups"""
    picks = [c for c in CASES if c["kind"] == "ok" and c["expected"] < 40000]
    many = [picks[(7 * i) % len(picks)] for i in range(600)]
    block, out_at, verdicts, produced, adlers = run_alone(many, 0)
    for c, at, v, n in zip(many, out_at, verdicts, produced):
        assert (v, n) == (OK, c["expected"]) and block[at:at + n].tobytes() == c["data"], c["name"]


# ---- the batch entries -----------------------------------------------------------------------------------------------------------
def routes(clear=True):
    from pixo_amd import jpeg
    return jpeg.debug_routes(clear=clear)


def same_with_and_without(files, what, redo=False, **kw):
    """decode_png_batch with the flag against the call without it; the route bits"""
    want = lib().decode_png_batch(files, **kw)
    routes()
    got = lib().decode_png_batch(files, device_inflate=True, **kw)
    bits = routes()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g.width, g.height, g.color_type) == (w.width, w.height, w.color_type), (what, i)
        assert g.pixels == w.pixels, "%s: image %d differs from the call without the flag" % (what, i)
    assert bits & BIT_DEVICE, what
    assert bool(bits & BIT_REDO) == redo, "%s: the host inflated %s" % (what, "nothing again" if redo else "a valid stream again")
    return got


def pass_rows():
    from pixo_amd import _lib
    return int(_lib.load().pixo_hip_png_unfilter_pass_rows())


def test_every_shape_and_layout():
    shapes = [f for _, f in PC.shape_cases(pass_rows())]
    got = same_with_and_without(shapes, "shapes")
    for im, f in zip(got, shapes):
        assert im.pixels == PC.model(f)[2]
    same_with_and_without([f for _, f in PC.layout_cases()], "layouts")
    split = [PC.make(33, 9, PC.RGB, 8, seed=43, idat_split=50), PC.make(129, 130, PC.RGBA, 8, seed=44, idat_split=1000),
             PC.make(67, 65, PC.INDEXED, 4, seed=45, idat_split=7, trns=bytes([0, 128])), PC.make(70, 1, PC.GRAY, 16, seed=46, idat_split=1)]
    same_with_and_without(split, "split IDATs")


def test_the_device_entry():
    import torch
    files = [f for _, f in PC.shape_cases(pass_rows())][::3] + [f for _, f in PC.layout_cases()][::4]
    want = lib().decode_png_batch_device(files)
    routes()
    got = lib().decode_png_batch_device(files, device_inflate=True)
    torch.cuda.synchronize()
    bits = routes()
    assert bits & BIT_DEVICE and not bits & BIT_REDO
    for i, ((g, gct), (w, wct)) in enumerate(zip(got, want)):
        assert gct == wct and g.shape == w.shape and torch.equal(g, w), i


def small(c):
    return c["w"] <= 129 and c["h"] <= 130


def test_the_librarys_own_encoders_files_at_both_efforts():
    """zlib never writes an over-subscribed set, and neither does the device DEFLATE: no file falls to the host"""
    from pixo_amd import ColorType, png
    files = []
    for c in [c for c in FC.CASES if small(c)]:
        px = FC.make_input(c)
        for flags in (png.NO_RAYON, png.NO_RAYON | png.EFFORT_HIGH):
            o = png.PngOptions.builder(c["w"], c["h"]).color_type(ColorType(c["color_type"])).preset(c["preset"]).flags(flags).build()
            files.append(png.encode(px, o))
    assert len(files) >= 40
    same_with_and_without(files, "own encoder")


def test_the_stored_whole_file_vectors():
    files = [FC.stored_file(c) for c in FC.CASES if c.get("stored") and small(c)]
    assert len(files) >= 30
    same_with_and_without(files, "stored vectors")


def with_idat(png, body):
    at = png.index(b"IDAT") - 4
    n = struct.unpack(">I", png[at:at + 4])[0]
    return png[:at] + PC.chunk(b"IDAT", body) + png[at + 12 + n:]


def idat_of(png):
    return b"".join(FC.parse(png)[0])


def phase_2_cases():
    good = PC.make(6, 5, PC.RGB, 8, seed=63)
    z = idat_of(good)
    errors = IC.error_streams()
    for message in sorted(set(errors) - set(IC.HEADER_ERRORS)):
        yield "stream_" + message.replace(" ", "_").replace("/", "_").replace(":", ""), with_idat(good, errors[message])
    yield "adler", with_idat(good, z[:-1] + bytes([z[-1] ^ 0x5A]))
    yield "size_short", with_idat(good, zlib.compress(zlib.decompress(z)[:-1]))
    yield "size_long", with_idat(good, zlib.compress(zlib.decompress(z) + b"\0"))
    yield "truncated", with_idat(good, z[:len(z) // 2] + z[-4:])
    yield "filter_7", PC.make(6, 5, PC.RGB, 8, filters=[0, 2, 7, 4, 9], seed=64)
    yield "missing_plte", PC.make(6, 5, PC.INDEXED, 8, seed=65, no_plte=True)


PHASE_2 = list(phase_2_cases())


def refusal(files, **kw):
    from pixo_amd import error
    with pytest.raises(error.Error) as e:
        lib().decode_png_batch(files, **kw)
    return type(e.value), str(e.value)


@pytest.mark.parametrize("name,png", PHASE_2, ids=[n for n, _ in PHASE_2])
def test_phase_2_refusals_equal_the_call_without_the_flag(name, png):
    import torch
    from pixo_amd import error
    good = [PC.make(40, 70, PC.RGB, 8, seed=130 + i) for i in range(2)]
    files = [good[0], png, good[1]]
    want = refusal(files)
    assert want[1].endswith(" (image 1)")
    if not name.startswith(("stream_", "truncated")):  # (the model has no words for an ill-formed DEFLATE body)
        assert want[1] == str(PC.model(png)) + " (image 1)"
    assert refusal(files, device_inflate=True) == want
    assert refusal(files, device_inflate=True, one_thread=True) == want
    with pytest.raises(error.Error) as e:
        lib().decode_png_batch_device(files, device_inflate=True)
    torch.cuda.synchronize()
    assert (type(e.value), str(e.value)) == want
    # the context survives
    assert lib().decode_png_batch(good, device_inflate=True) == lib().decode_png_batch(good)


def test_of_two_broken_files_the_lower_index_decides():
    good = PC.make(40, 70, PC.RGB, 8, seed=140)
    by_name = dict(PHASE_2)
    for a, b in (("adler", "filter_7"), ("filter_7", "adler"), ("missing_plte", "stream_invalid_distance_code"), ("size_short", "missing_plte")):
        files = [good, by_name[a], good, by_name[b], good]
        want = refusal(files)
        assert want[1].endswith(" (image 1)")
        assert refusal(files, device_inflate=True) == want
    try:
        from pixo_amd import jpeg
        jpeg.debug_configure("decode_batch_bytes=1")  # every file a sub-batch of its own: the second broken file is never reached
        assert refusal([good, by_name["adler"], good, by_name["filter_7"]], device_inflate=True) == refusal([good, by_name["adler"]])
    finally:
        jpeg.debug_configure(None)


def oversubscribed_png(count=4):
    """A 3x1 gray image whose IDAT stream has an over-subscribed literal set the host inflate decodes (inflate_cases.py): four bytes
    of value 2 — filter Up over nothing, three pixels of 2"""
    z, data = IC.oversubscribed_stream(count)
    assert data == bytes([2]) * 4
    return M.SIGNATURE + PC.chunk(b"IHDR", PC.ihdr(3, 1, 8, PC.GRAY)) + PC.chunk(b"IDAT", z) + PC.chunk(b"IEND", b"")


def test_an_oversubscribed_stream_is_the_hosts():
    png = oversubscribed_png()
    single = lib().decode_png(png)
    assert (single.width, single.height, single.pixels) == (3, 1, bytes([2, 2, 2]))
    got = same_with_and_without([png], "over-subscribed alone", redo=True)
    assert got[0].pixels == single.pixels
    good = [PC.make(67, 65, PC.RGB, 8, seed=150), PC.make(33, 70, PC.INDEXED, 4, seed=151, trns=bytes([0, 128]))]
    for kw in (dict(), dict(one_thread=True)):
        got = same_with_and_without([good[0], png, good[1], png], "over-subscribed among others", redo=True, **kw)
        assert got[1].pixels == got[3].pixels == single.pixels
    same_with_and_without(good, "and none after it")


def test_sub_batches_give_the_same_pixels():
    from pixo_amd import jpeg
    files = [PC.make(w, h, ct, d, seed=140 + i, trns=PC.trns_for(ct, d, w))
             for i, (w, h, ct, d) in enumerate([(67, 65, PC.RGB, 8), (33, 70, PC.RGBA, 8), (129, 3, PC.INDEXED, 4), (16, 131, PC.GRAY, 8),
                                                (70, 67, PC.RGB, 8), (5, 5, PC.GRAY_ALPHA, 16)])]
    files.insert(3, oversubscribed_png())
    uncut = lib().decode_png_batch(files)
    try:
        for limit, cuts in ((30000, 3), (1, 7)):
            jpeg.debug_configure("decode_batch_bytes=%d" % limit)
            assert len(lib().decode_png_batch_plan(files)["sub_first"]) == cuts + 1
            routes()
            assert lib().decode_png_batch(files, device_inflate=True) == uncut
            bits = routes()
            assert bits & BIT_DEVICE and bits & BIT_REDO and bits & jpeg.ROUTE_SUB_BATCHES
    finally:
        jpeg.debug_configure(None)
    assert lib().decode_png_batch(files, device_inflate=True) == uncut


def test_d_pixels_at_odd_addresses():
    import torch
    files = [PC.make(1, 1, PC.GRAY, 8, seed=111), PC.make(5, 3, PC.RGB, 8, seed=112), PC.make(64, 4, PC.RGBA, 8, seed=113),
             PC.make(9, 5, PC.INDEXED, 4, seed=114, trns=bytes([0, 128])), PC.make(16, 70, PC.GRAY, 8, seed=115), PC.make(67, 65, PC.RGB, 16, seed=116)]
    info, total = lib().decode_png_batch_info(files)
    for shift in (0, 1, 3):
        big = torch.full((total + 64 + shift,), 0xA5, dtype=torch.uint8, device="cuda")
        lib().decode_png_batch_device(files, out=big[shift:], device_inflate=True)
        torch.cuda.synchronize()
        host = big.cpu().numpy()
        written = np.zeros(host.size, bool)
        for png, (w, h, ct, offset) in zip(files, info):
            want = PC.model(png)[2]
            assert host[shift + offset:shift + offset + len(want)].tobytes() == want, shift
            written[shift + offset:shift + offset + len(want)] = True
        assert (host[~written] == 0xA5).all(), shift


def test_one_thread_and_call_histories():
    files = [f for _, f in PC.shape_cases(pass_rows())][::7]
    want = lib().decode_png_batch(files)
    assert lib().decode_png_batch(files, one_thread=True, device_inflate=True) == want
    big = [PC.make(150 + i, 140, (PC.RGBA, PC.INDEXED, PC.GRAY, PC.RGB)[i % 4], 8, seed=160 + i, trns=bytes([9]) if i % 4 == 1 else None) for i in range(9)]
    for batch in (big, files[:2], big[:3]):  # buffers regrow and shrink in use between calls with and without the flag
        assert lib().decode_png_batch(batch, device_inflate=True) == lib().decode_png_batch(batch)
    assert lib().decode_png(files[0]).pixels == want[0].pixels
