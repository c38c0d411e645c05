"""PNG decode batches on the device (pixo_hip_png_decode_batch*, png_unfilter.hip's batch kernels): every image of a batch
against the sequential model (tests/png_decode_model.py) and against the single entry, at the sizes where the kernels'
structure can go wrong — every colour type, depth and filter unit in one call, runs across pass boundaries, every filter
layout —, the gaps between images and unaligned caller storage, the device pipeline decode batch -> resize batch -> JPEG
batch without a host wait, capacity, a phase-2 refusal, sub-batches, the thread flag, call histories and calling threads."""
import threading

import numpy as np
import pytest

import png_decode_cases as PC
import png_decode_model as M

pytestmark = pytest.mark.gpu


def lib():
    from pixo_amd import decode
    return decode


def pass_rows():
    from pixo_amd import _lib  # (the pass height is the kernel's own constant)
    return int(_lib.load().pixo_hip_png_unfilter_pass_rows())


SHAPES = list(PC.shape_cases(pass_rows()))
LAYOUTS = list(PC.layout_cases())


def same_as_model(images, cases, singles=False, what=""):
    """images: [PngImage] of the files of cases [(name, file)]"""
    from pixo_amd import ColorType
    assert len(images) == len(cases)
    for im, (name, png) in zip(images, cases):
        want = PC.model(png)
        assert not isinstance(want, Exception), (name, want)
        assert (im.width, im.height, im.color_type) == (want[0], want[1], ColorType(want[3])), (what, name)
        assert im.pixels == want[2], "%s %s: pixels differ from the model's" % (what, name)
        if singles:
            one = lib().decode_png(png)
            assert (one.width, one.height, one.pixels, one.color_type) == (im.width, im.height, im.pixels, im.color_type), (what, name)


def test_every_shape_in_one_call():
    """Every colour type x depth x size, the filter units mixed in index order: all six unfilter launches and the byte-wise and
    sample-wise convert launches serve images scattered over the batch"""
    p = lib().decode_png_batch_plan([f for _, f in SHAPES])
    # (no row of these sizes is a multiple of 16 bytes: the 16-byte convert form is test_gaps_and_caller_alignment's)
    assert p["unfilter_launches"] == 6 and p["convert_launches"] == 2 and p["sub_first"] == [0, len(SHAPES)]
    same_as_model(lib().decode_png_batch([f for _, f in SHAPES]), SHAPES, singles=True, what="shapes")


def test_every_filter_layout_in_one_call():
    p = lib().decode_png_batch_plan([f for _, f in LAYOUTS])
    assert max(p["runs"]) >= 3 and min(p["runs"]) == 1
    same_as_model(lib().decode_png_batch([f for _, f in LAYOUTS]), LAYOUTS, singles=True, what="layouts")


def test_small_and_repeated_batches():
    one = ("one", PC.make(67, 65, PC.RGB, 8, seed=101))
    same_as_model(lib().decode_png_batch([one[1]]), [one], what="batch of one")
    same_as_model(lib().decode_png_batch([one[1]] * 3), [one] * 3, what="the same file three times")
    pal = [("rgba", PC.make(33, 70, PC.INDEXED, 4, seed=102, trns=bytes([0, 128, 7]))),
           ("rgb", PC.make(70, 33, PC.INDEXED, 8, seed=103, plte_entries=200, trns=bytes([255, 255])))]
    got = lib().decode_png_batch([f for _, f in pal])
    assert [int(im.color_type) for im in got] == [3, 2]
    same_as_model(got, pal, what="two palettes")


def mixed_files():
    return [("gray1x1", PC.make(1, 1, PC.GRAY, 8, seed=111)), ("rgb5x3", PC.make(5, 3, PC.RGB, 8, seed=112)),
            ("rgba64x4", PC.make(64, 4, PC.RGBA, 8, seed=113)), ("pal", PC.make(9, 5, PC.INDEXED, 4, seed=114, trns=bytes([0, 128]))),
            ("gray16x70", PC.make(16, 70, PC.GRAY, 8, seed=115)), ("rgb16", PC.make(67, 65, PC.RGB, 16, seed=116)),
            ("gray2", PC.make(13, 7, PC.GRAY, 2, seed=117)), ("rgba4x3", PC.make(4, 3, PC.RGBA, 8, seed=118))]


def test_gaps_and_caller_alignment():
    """Nothing but the images' own bytes is written: the gaps between them and the bytes behind the total keep their 0xA5, also
    when `out` starts 1, 2 or 3 bytes into a larger tensor (the 16-byte and dword stores are chosen by the real address)"""
    import torch
    files = mixed_files()
    info, total = lib().decode_png_batch_info([f for _, f in files])
    assert lib().decode_png_batch_plan([f for _, f in files])["convert_launches"] == 3  # the 16-byte form too, where `out` is aligned
    for shift in (0, 1, 2, 3):
        big = torch.full((total + 64 + shift,), 0xA5, dtype=torch.uint8, device="cuda")
        out = big[shift:]
        views = lib().decode_png_batch_device([f for _, f in files], out=out)
        torch.cuda.synchronize()
        host = big.cpu().numpy()
        written = np.zeros(host.size, bool)
        for (t, ct), (name, png), (w, h, ict, offset) in zip(views, files, info):
            want = PC.model(png)
            assert (t.shape[1], t.shape[0], int(ct)) == (want[0], want[1], want[3]) and ct == ict, (shift, name)
            assert t.data_ptr() == out.data_ptr() + offset and offset % 16 == 0
            assert host[shift + offset:shift + offset + len(want[2])].tobytes() == want[2], (shift, name)
            written[shift + offset:shift + offset + len(want[2])] = True
        assert written.sum() < host.size - 64 - shift and (host[~written] == 0xA5).all(), shift


def test_device_pipeline_decode_resize_encode_without_a_host_wait():
    import torch
    from pixo_amd import ColorType, jpeg, resize
    sizes = [(129, 130), (67, 65), (33, 131), (129, 130)]
    files = [PC.make(w, h, PC.RGB, 8, seed=120 + i) for i, (w, h) in enumerate(sizes)]
    pixels = [np.frombuffer(PC.model(f)[2], np.uint8) for f in files]
    dw, dh = 64, 48
    jopts = jpeg.JpegOptions.builder(dw, dh).color_type(ColorType.Rgb).quality(80).subsampling(jpeg.Subsampling.S420).build()
    want_small = resize.resize_batch([(px, w, h) for px, (w, h) in zip(pixels, sizes)], dw, dh, 2, 2)
    want_jpeg = [jpeg.encode(np.frombuffer(s, np.uint8), jopts) for s in want_small]
    side = torch.cuda.Stream()
    before = jpeg.get_producer_stream()
    try:
        with torch.cuda.stream(side):
            jpeg.set_producer_stream(side.cuda_stream)
            d_small = torch.empty(len(files) * dw * dh * 3, dtype=torch.uint8, device="cuda")
            views = lib().decode_png_batch_device(files, stream=side.cuda_stream)
            resize.resize_batch_device([(t, t.shape[1], t.shape[0]) for t, _ in views], dw, dh, 2, 2, d_small, side.cuda_stream)
            got_jpeg = jpeg.encode_batch_device(d_small, jopts, len(files))  # (ordered behind the producer stream by the library)
            side.synchronize()
    finally:
        jpeg.set_producer_stream(before)
    assert all(ct == ColorType.Rgb for _, ct in views)
    assert d_small.cpu().numpy().tobytes() == b"".join(want_small) and got_jpeg == want_jpeg


def test_too_small_a_capacity_says_what_is_needed():
    import torch
    from pixo_amd import error
    files = mixed_files()
    _, total = lib().decode_png_batch_info([f for _, f in files])
    with pytest.raises(error.BufferTooSmall) as e:
        lib().decode_png_batch_device([f for _, f in files], out=torch.empty(total - 1, dtype=torch.uint8, device="cuda"))
    assert e.value.needed == total and str(e.value) == "output buffer too small: need %d bytes" % total
    views = lib().decode_png_batch_device([f for _, f in files], out=torch.empty(total, dtype=torch.uint8, device="cuda"))
    for (t, _), (name, png) in zip(views, files):
        assert t.cpu().numpy().tobytes() == PC.model(png)[2], name


def test_a_phase_2_refusal_leaves_out_untouched_and_the_context_survives():
    import torch
    from pixo_amd import error
    good = [PC.make(40, 70, PC.RGB, 8, seed=130 + i) for i in range(3)]
    bad = PC.make(40, 70, PC.RGB, 8, filters=[0] * 69 + [6], seed=133)
    want = PC.model(bad)
    assert isinstance(want, M.DecodeError)
    _, total = lib().decode_png_batch_info(good[:2] + [bad] + good[2:])
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(error.InvalidDecode) as e:
        lib().decode_png_batch_device(good[:2] + [bad] + good[2:], out=out)
    assert str(e.value) == str(want) + " (image 2)"
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()
    with pytest.raises(error.InvalidDecode) as e:
        lib().decode_png_batch(good[:2] + [bad] + good[2:])
    assert str(e.value) == str(want) + " (image 2)"
    same_as_model(lib().decode_png_batch(good), [("good", f) for f in good], what="after the refusal")


def test_sub_batches_give_the_same_block():
    from pixo_amd import jpeg
    cases = [("c%d" % i, PC.make(w, h, ct, d, seed=140 + i, trns=PC.trns_for(ct, d, w)))
             for i, (w, h, ct, d) in enumerate([(67, 65, PC.RGB, 8), (33, 70, PC.RGBA, 8), (129, 3, PC.INDEXED, 4), (16, 131, PC.GRAY, 8),
                                                (70, 67, PC.RGB, 8), (5, 5, PC.GRAY_ALPHA, 16)])]
    files = [f for _, f in cases]
    jpeg.debug_routes(clear=True)
    uncut = lib().decode_png_batch(files)
    bits = jpeg.debug_routes(clear=True)
    assert bits & lib().ROUTE_PNG_DECODE_BATCH and not bits & jpeg.ROUTE_SUB_BATCHES
    same_as_model(uncut, cases, what="uncut")
    try:
        jpeg.debug_configure("decode_batch_bytes=30000")  # the staging: 26656 19392 448 4336 29152 272 bytes
        assert lib().decode_png_batch_plan(files)["sub_first"] == [0, 1, 4, 6]
        cut = lib().decode_png_batch(files)
        bits = jpeg.debug_routes(clear=True)
        assert bits & lib().ROUTE_PNG_DECODE_BATCH and bits & jpeg.ROUTE_SUB_BATCHES
        assert cut == uncut
        jpeg.debug_configure("decode_batch_bytes=1")
        assert lib().decode_png_batch(files) == uncut
    finally:
        jpeg.debug_configure(None)
    assert lib().decode_png_batch_plan(files)["sub_first"] == [0, 6]


def test_one_thread_equals_the_pool():
    files = [f for _, f in SHAPES[::7]] + [f for _, f in LAYOUTS[::5]]
    assert lib().decode_png_batch(files, one_thread=True) == lib().decode_png_batch(files)


def test_call_histories_regrow_buffers_and_leave_no_stale_tables():
    a = [("a%d" % i, PC.make(20 + i, 9, PC.INDEXED, 8, seed=150 + i, trns=bytes([i, 200]))) for i in range(3)]
    single = PC.make(300, 200, PC.RGB, 8, seed=154)
    big = [("b%d" % i, PC.make(150 + i, 140, (PC.RGBA, PC.INDEXED, PC.GRAY, PC.RGB)[i % 4], 8, seed=160 + i, trns=bytes([9]) if i % 4 == 1 else None))
           for i in range(9)]
    small = [("s%d" % i, PC.make(7, 3 + i, PC.INDEXED, 2, seed=170 + i)) for i in range(2)]
    same_as_model(lib().decode_png_batch([f for _, f in a]), a, what="first batch")
    one = lib().decode_png(single)
    assert one.pixels == PC.model(single)[2]
    same_as_model(lib().decode_png_batch([f for _, f in big]), big, what="larger batch")
    same_as_model(lib().decode_png_batch([f for _, f in small]), small, what="smaller batch")
    assert lib().decode_png(single).pixels == one.pixels


def test_three_calling_threads():
    sets = [[("t0_%d" % i, PC.make(90 + i, 70, PC.RGB, 8, seed=180 + i)) for i in range(3)],
            [("t1_%d" % i, PC.make(40, 66 + i, PC.INDEXED, 2, seed=184 + i, trns=bytes([3]))) for i in range(4)],
            [("t2_%d" % i, PC.make(64, 20 + i, PC.GRAY_ALPHA, 16, seed=190 + i)) for i in range(2)]]
    for s in sets:
        for _, f in s:
            PC.model(f)  # (computed once, on this thread)
    errors = []

    def work(i):
        try:
            for _ in range(3):
                same_as_model(lib().decode_png_batch([f for _, f in sets[i]]), sets[i], what="thread %d" % i)
        except BaseException as e:  # noqa: BLE001
            errors.append((i, e))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
