"""JPEG decode on the device (`decode.decode_jpeg*`).  Every case of tests/jpeg_decode_cases.py — files written by Pillow,
with the pixels libjpeg-turbo decodes from them committed — must come back byte for byte through the single entries and the
batch entries; a batch image must be the single entry's; d_pixels at odd addresses; sentinels in the gaps, in front of the
block and behind it; a refusal in file k; restart intervals written by this library's own encoder; and the chain into resize
and encode."""
import ctypes as C
import io

import numpy as np
import pytest

import jpeg_decode_cases as JC
import jpeg_decode_model as M
import synth

pytestmark = pytest.mark.gpu


def D():
    from pixo_amd import decode
    return decode


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("c", JC.CASES, ids=JC.IDS)
def test_single_entries_give_libjpeg_pixels(c):
    from pixo_amd import ColorType
    d = D()
    im = d.decode_jpeg(JC.data(c))
    assert (im.width, im.height, im.color_type) == (c["w"], c["h"], ColorType(c["color_type"]))
    assert JC.mismatch(im.pixels, c) == ""
    t, ct = d.decode_jpeg_device(JC.data(c))
    assert tuple(t.shape) == (c["h"], c["w"], c["color_type"] + 1) and ct == ColorType(c["color_type"])
    assert JC.mismatch(host(t), c) == ""


def test_batch_of_every_case_mixes_all_classes_in_four_launches():
    d = D()
    files = [JC.data(c) for c in JC.CASES]
    plan = d.decode_jpeg_batch_plan(files)
    assert set(plan["classes"]) == set(d.JPEG_CLASSES) and plan["launches"] == 4 and plan["sub_first"] == [0, len(files)]
    views = d.decode_jpeg_batch_device(files)
    for c, (t, ct) in zip(JC.CASES, views):
        assert JC.mismatch(host(t), c) == ""
    images = d.decode_jpeg_batch(files)
    one = d.decode_jpeg_batch(files, one_thread=True)
    for c, im, im1 in zip(JC.CASES, images, one):
        assert JC.mismatch(im.pixels, c) == "" and im1 == im
        assert (im.width, im.height, int(im.color_type)) == (c["w"], c["h"], c["color_type"])


def test_batch_image_is_the_single_entrys():
    d = D()
    cases = JC.small()[::3]
    views = d.decode_jpeg_batch_device([JC.data(c) for c in cases])
    for c, (t, _) in zip(cases, views):
        assert host(t) == d.decode_jpeg(JC.data(c)).pixels


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_any_alignment_and_nothing_written_outside_the_images(offset):
    """d_pixels at offsets 0, 1 and 3 from an aligned block: the byte form at odd addresses.  A pattern in front of the block,
    in the gaps between images and behind the block must survive."""
    import torch
    d = D()
    cases = [JC.by_name(n) for n in ("gray_7x5_q80", "420_17x17_q80", "444_9x9_q80", "422_33x17_q80", "420_1x1_q80", "gray_50x37_q80", "420_50x37_q80",
                                     "422_50x37_q80_rst5")] + [c for c in JC.CASES if c.get("tile")]
    files = [JC.data(c) for c in cases]
    layout, total = d.decode_jpeg_batch_info(files)
    pad = 64
    pattern = np.frombuffer(synth.lcg_bytes(pad + offset + total + pad, 77).tobytes(), np.uint8).copy()
    block = torch.from_numpy(pattern.copy()).cuda()
    views = d.decode_jpeg_batch_device(files, out=block[pad + offset:pad + offset + total])
    got = np.frombuffer(host(block), np.uint8)
    want = pattern.copy()
    for c, (w, h, ct, at) in zip(cases, layout):
        assert at % 16 == 0
        want[pad + offset + at:pad + offset + at + len(JC.expected(c))] = np.frombuffer(JC.expected(c), np.uint8)
    assert np.array_equal(got[:pad + offset], want[:pad + offset]), "bytes in front of the block changed"
    assert np.array_equal(got[pad + offset + total:], want[pad + offset + total:]), "bytes behind the block changed"
    for c, (t, _) in zip(cases, views):
        assert JC.mismatch(host(t), c) == ""
    assert np.array_equal(got, want), "bytes between the images changed"


@pytest.mark.parametrize("broken", ["walk", "scan"])
def test_refusal_in_file_k_leaves_images_and_pixels_untouched(broken):
    import torch
    from pixo_amd import _lib, error
    d = D()
    good = [JC.data(JC.by_name(n)) for n in ("420_17x17_q80", "gray_9x9_q80", "444_16x16_q80")]
    bad = JC.data(JC.by_name("420_50x37_q80"))
    bad = bad[:2] + b"\xff\xc2\x00\x02" + bad[2:] if broken == "walk" else bad[:-40]
    files = good[:2] + [bad] + good[2:]
    message = "Unsupported: progressive JPEG not supported (image 2)" if broken == "walk" else "Decode error: entropy-coded segment ends early (image 2)"
    block = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
    arr, held = d._files_c(files)
    images = (_lib.PngImageC * 4)()
    for im in images:
        im.offset, im.width = 0xDEAD, 0xBEEF
    rc = _lib.load().pixo_hip_jpeg_decode_batch_device(arr, 4, 0, block.data_ptr(), block.numel(), images, None)
    assert rc in (-10, -11) and _lib.load().pixo_hip_last_error().decode() == message
    if broken == "walk":
        assert all(im.offset == 0xDEAD and im.width == 0xBEEF for im in images)
    assert set(host(block)) == {0x5A}, "something was enqueued"
    with pytest.raises(error.Error, match="image 2"):
        d.decode_jpeg_batch(files)
    # the same thread's next call is sound
    assert JC.mismatch(d.decode_jpeg(good[0]).pixels, JC.by_name("420_17x17_q80")) == ""
    # the single entry's refusal carries no index
    with pytest.raises(error.Error) as e:
        d.decode_jpeg(bad)
    assert str(e.value) == message[:-len(" (image 2)")]


@pytest.mark.parametrize("ct,ss", [(0, 0), (2, 0), (2, 1)], ids=["gray", "444", "420"])
def test_restart_intervals_written_by_this_librarys_encoder(ct, ss):
    """Intervals of 1 MCU, one MCU row and a number that divides nothing; the expectation is the sequential model's (which the
    CPU tests hold against Pillow), and live Pillow's where it is built on libjpeg-turbo."""
    from PIL import Image, features
    from pixo_amd import ColorType, jpeg
    d = D()
    w, h = 50, 37
    px = synth.scene(w, h, 31).reshape(h, w, 3)
    px = np.ascontiguousarray(px[:, :, 1]) if ct == 0 else px
    row = -(-w // (16 if ss else 8))
    for interval in (1, row, 7):
        o = jpeg.JpegOptions.builder(w, h).color_type(ColorType(ct)).quality(85).subsampling(jpeg.Subsampling(ss)).restart_interval(interval).build()
        f = jpeg.encode(px.reshape(-1), o)
        assert b"\xff\xdd" in f
        want = M.decode(f)[2].tobytes()
        if features.check_feature("libjpeg_turbo"):
            assert np.asarray(Image.open(io.BytesIO(f))).tobytes() == want
        assert d.decode_jpeg(f).pixels == want, (ct, ss, interval)


def test_sub_batches_by_the_debug_switch():
    """A limit of 64 KiB of coefficients a sub-batch: the batch is cut, every image is still the expectation."""
    from pixo_amd import jpeg
    d = D()
    cases = [c for c in JC.CASES if c["w"] == 50][:12]
    files = [JC.data(c) for c in cases]
    jpeg.debug_configure("decode_batch_bytes=65536")
    try:
        plan = d.decode_jpeg_batch_plan(files)
        views = d.decode_jpeg_batch_device(files)
        got = [host(t) for t, _ in views]
    finally:
        jpeg.debug_configure("")
    assert len(plan["sub_first"]) > 2
    for c, g in zip(cases, got):
        assert JC.mismatch(g, c) == ""


def test_chain_decode_fit_resize_encode():
    """decode batch -> fit_images -> resize_images_device -> jpeg.encode_images_device, against the same chain fed with the
    expected pixels uploaded by hand in the same layout."""
    import torch
    from pixo_amd import ColorType, jpeg, resize
    d = D()
    cases = [JC.by_name(n) for n in ("420_50x37_q80", "gray_50x37_q95", "444_33x17_q80", "422_50x37_q30")]
    files = [JC.data(c) for c in cases]
    layout, total = d.decode_jpeg_batch_info(files)
    block = np.zeros(total, np.uint8)
    for c, (w, h, ct, at) in zip(cases, layout):
        block[at:at + len(JC.expected(c))] = np.frombuffer(JC.expected(c), np.uint8)
    o = jpeg.JpegOptions.builder(0, 0).color_type(ColorType.Rgb).quality(80).subsampling(jpeg.Subsampling(1)).build()

    def tail(d_src, records):
        fitted, n = resize.fit_images(records, 24, 24)
        d_dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
        resize.resize_images_device(d_src, records, d_dst, fitted, resize.ResizeAlgorithm.Bilinear)
        torch.cuda.synchronize()
        return jpeg.encode_images_device(d_dst, fitted, o)

    views = d.decode_jpeg_batch_device(files)
    got = tail(None, views)
    want = tail(torch.from_numpy(block).cuda(), layout)
    assert len(got) == 4 and got == want
