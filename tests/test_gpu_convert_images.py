"""The colour-conversion images entries on the GPU (pixo_hip_convert_images*): image i byte for byte the model's
(tests/convert_model.py) and the single entry's, the bytes between destinations untouched — one image, two, all five kinds
and both forms in one call, 300 seeded images for both targets, 65535 one-pixel images, a batch cut into three sub-batches,
a call behind calls with larger and smaller tables, the host-block entry — and the chain the entries exist for: decode batch
-> fit -> resize images -> convert images -> JPEG images (OPAQUE) or PNG images (GRAY)."""
import random

import numpy as np
import pytest

import convert_cases as CC
import convert_model as M

pytestmark = pytest.mark.gpu


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(src_records, block, dst_records, total, s_off=0, d_off=0):
    """The block at s_off, the destinations' block at d_off modulo 16 -> the destinations' block, filled with AFTER before"""
    import torch
    from pixo_amd import convert
    d_src = torch.empty(block.size + 16, dtype=torch.uint8, device="cuda")
    d_src[s_off:s_off + block.size] = cuda(block)
    d_dst = torch.full((total + 16,), CC.AFTER, dtype=torch.uint8, device="cuda")
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    convert.convert_images_device(d_src[s_off:], src_records, d_dst[d_off:], dst_records)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.all(got[:d_off] == CC.AFTER) and np.all(got[d_off + total:] == CC.AFTER)
    return got[d_off:d_off + total]


def check_against_single_entry(got, block, src_records, dst_records):
    import torch
    from pixo_amd import convert
    for i, (s, d) in enumerate(zip(src_records, dst_records)):
        d_one = torch.empty(max(d[0] * d[1] * M.bpp(int(d[2])), 1), dtype=torch.uint8, device="cuda")
        convert.convert_device(cuda(CC.image_bytes(block, s)), s[0], s[1], int(s[2]), int(d[2]), d_one)
        torch.cuda.synchronize()
        assert np.array_equal(CC.image_bytes(got, d), d_one.cpu().numpy()), "image %d differs from the single entry's" % i


def test_one_image_and_two():
    from pixo_amd import convert
    for shapes in ([(37, 23, M.RGBA)], [(64, 65, M.GRAY_ALPHA), (5, 3, M.RGBA)]):
        src, block = CC.block_of(shapes, 500)
        for target in (convert.Target.OPAQUE, convert.Target.GRAY):
            dst, total = convert.layout_images(src, target)
            got = run(src, block, dst, total)
            CC.check_block(got, block, src, dst)
            check_against_single_entry(got, block, src, dst)


def test_all_kinds_and_both_forms_in_one_call():
    from pixo_amd import convert
    t = convert.tile_pixels()
    pairs = [(M.RGB, M.RGB), (M.GRAY_ALPHA, M.GRAY), (M.RGBA, M.RGB), (M.RGB, M.GRAY), (M.RGBA, M.GRAY)]
    sizes = [(33, 31), (t + 1, 1), (17, 1), (64, 65), (t, 2), (15, 1), (1, 1), (129, 7), (16, 1), (t - 1, 3), (40, 40)]
    shapes = [(w, h, pairs[i % 5][0]) for i, (w, h) in enumerate(sizes)]
    odd_src, odd_dst = {1, 2, 9}, {3, 5, 9}  # every kind (image index % 5) once or twice aligned on both sides, once not
    src, block = CC.block_of(shapes, 520, odd=odd_src)
    dst, total = CC.destinations(src, [pairs[i % 5][1] for i in range(len(sizes))], odd=odd_dst)
    plan = convert.convert_images_plan(src, dst)
    assert plan["kind"] == [i % 5 for i in range(11)] and plan["form"] == [int(i in odd_src | odd_dst) for i in range(11)]
    assert plan["launches"] == len({(k, f) for k, f in zip(plan["kind"], plan["form"])}) == 10
    got = run(src, block, dst, total)
    CC.check_block(got, block, src, dst)
    check_against_single_entry(got, block, src, dst)
    # the same records in blocks that are themselves odd: every image takes the byte form
    assert set(convert.convert_images_plan(src, dst, 3, 0)["form"]) | set(convert.convert_images_plan(src, dst, 0, 5)["form"]) <= {0, 1}
    CC.check_block(run(src, block, dst, total, s_off=3, d_off=5), block, src, dst)


@pytest.mark.parametrize("target", (M.OPAQUE, M.TO_GRAY), ids=("opaque", "gray"))
def test_300_seeded_images(target):
    from pixo_amd import convert
    rnd = random.Random(530 + target)
    shapes = [(rnd.randint(1, 40), rnd.randint(1, 40), rnd.randrange(4)) for _ in range(300)]
    src, block = CC.block_of(shapes, 540, odd={i for i in range(300) if rnd.random() < 0.2})
    dst, total = convert.layout_images(src, target)
    assert [int(d[2]) for d in dst] == [M.target_type(target, ct) for _, _, ct in shapes]
    CC.check_block(run(src, block, dst, total), block, src, dst)


def test_65535_images_of_one_pixel():
    from pixo_amd import convert
    n = 65535
    cts = np.random.default_rng(550).integers(0, 4, n)
    src = [(1, 1, int(ct), 16 * i) for i, ct in enumerate(cts)]
    block = np.random.default_rng(551).integers(0, 256, 16 * n, dtype=np.uint8)
    dst, total = convert.layout_images(src, convert.Target.GRAY)
    assert total == 16 * (n - 1) + 1
    got = run(src, block, dst, total)
    px = block.reshape(n, 16)
    r, g, b = (px[:, k].astype(np.uint32) for k in range(3))
    luma = ((77 * r + 150 * g + 29 * b + 128) >> 8).astype(np.uint8)
    want = np.where(cts >= 2, luma, px[:, 0])
    padded = np.concatenate([got, np.full(15, CC.AFTER, np.uint8)]).reshape(n, 16)
    assert np.array_equal(padded[:, 0], want) and np.all(padded[:, 1:] == CC.AFTER)


def test_three_sub_batches_under_the_debug_switch():
    from pixo_amd import _lib, convert
    L = _lib.load()
    t = convert.tile_pixels()
    shapes = [(t, 5, M.RGBA), (t + 3, 5, M.RGBA), (t, 5, M.RGB), (t, 5, M.RGBA), (t - 1, 5, M.RGBA), (9, 9, M.RGB), (t, 5, M.RGBA), (t + 16, 5, M.RGBA)]
    src, block = CC.block_of(shapes, 560, odd={4})
    dst, total = convert.layout_images(src, convert.Target.OPAQUE)
    try:
        L.pixo_hip_debug_configure(b"convert_images_tiles=2")
        # (images 0 1 | 3 and 4 are of different forms, so they share a sub-batch with 6 | 7: two Rgba -> Rgb aligned images fill a launch)
        assert convert.convert_images_plan(src, dst)["sub_first"] == [0, 3, 7, 8]
        got = run(src, block, dst, total)
    finally:
        L.pixo_hip_debug_configure(None)
    CC.check_block(got, block, src, dst)
    assert np.array_equal(got, run(src, block, dst, total))  # ... and the bytes of the call without the switch


def test_a_call_behind_calls_with_a_larger_and_a_smaller_table():
    """The records' buffers are reused: 40 images, then 400 (they grow), then 3, back to back without a wait between them"""
    import torch
    from pixo_amd import convert
    jobs = []
    for n, seed in ((40, 570), (400, 571), (3, 572)):
        rnd = random.Random(seed)
        shapes = [(rnd.randint(1, 70), rnd.randint(1, 70), rnd.randrange(4)) for _ in range(n)]
        src, block = CC.block_of(shapes, seed)
        dst, total = convert.layout_images(src, convert.Target.OPAQUE)
        jobs.append((src, block, dst, cuda(block), torch.full((total,), CC.AFTER, dtype=torch.uint8, device="cuda")))
    torch.cuda.synchronize()
    for src, _, dst, d_src, d_dst in jobs:
        convert.convert_images_device(d_src, src, d_dst, dst)
    torch.cuda.synchronize()
    for src, block, dst, _, d_dst in jobs:
        CC.check_block(d_dst.cpu().numpy(), block, src, dst)


def test_the_host_block_entry():
    from pixo_amd import convert
    shapes = [(37, 23, M.RGBA), (64, 41, M.GRAY_ALPHA), (1, 1, M.GRAY), (129, 7, M.RGB), (5, 300, M.RGBA)]
    src, block = CC.block_of(shapes, 580, odd={3})
    for target in (convert.Target.OPAQUE, convert.Target.GRAY):
        dst, _ = convert.layout_images(src, target)
        got = convert.convert_images(block, src, dst)
        for i, (s, d) in enumerate(zip(src, dst)):
            assert got[i] == M.convert(CC.image_bytes(block, s), s[2], int(d[2])).tobytes(), i
        assert got == convert.convert_images(block.tobytes(), src, dst)


# ---- the chain ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_files():
    import png_decode_cases as DC
    files = [DC.make(67, 65, DC.GRAY, 8, seed=21), DC.make(70, 33, DC.GRAY_ALPHA, 8, seed=22), DC.make(129, 130, DC.RGB, 8, seed=23),
             DC.make(40, 90, DC.RGBA, 8, seed=24), DC.make(67, 65, DC.INDEXED, 4, seed=25, trns=bytes([0, 128]))]
    decoded = [DC.model(f) for f in files]  # (w, h, pixels, colour type)
    assert [int(d[3]) for d in decoded] == [M.GRAY, M.GRAY_ALPHA, M.RGB, M.RGBA, M.RGBA]
    return files, decoded


@pytest.mark.parametrize("target", (M.OPAQUE, M.TO_GRAY), ids=("opaque_to_jpeg", "gray_to_png"))
def test_chain_decode_fit_resize_convert_encode(chain_files, target):
    import torch
    from pixo_amd import ColorType, convert, decode, jpeg, png, resize
    files, decoded = chain_files
    algo = resize.ResizeAlgorithm.Lanczos3
    views = decode.decode_png_batch_device(files)
    fitted, total = resize.fit_images(views, 24, 24)
    d_small = torch.empty(total, dtype=torch.uint8, device="cuda")
    resize.resize_images_device(None, views, d_small, fitted, algo)
    laid, total = convert.layout_images(fitted, target)
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
    convert.convert_images_device(d_small, fitted, d_out, laid)
    if target == M.OPAQUE:
        got = jpeg.encode_images_device(d_out, laid, jpeg.JpegOptions.builder(0, 0).color_type(ColorType.Rgb).quality(80).build())
    else:
        got = png.encode_images_device(d_out, laid, png.PngOptions.builder(0, 0).preset(0).build())
    assert len(got) == len(files)
    for i, ((sw, sh, px, ct), (w, h, fct, _), (_, _, dct, _)) in enumerate(zip(decoded, fitted, laid)):
        assert max(w, h) == 24 and int(fct) == int(ct) and int(dct) == M.target_type(target, int(ct))
        small = resize.resize(np.frombuffer(px, np.uint8), resize.ResizeOptions.builder(sw, sh).dst(w, h).color_type(ColorType(int(ct))).algorithm(algo).build())
        want = M.convert(np.frombuffer(small, np.uint8), int(ct), int(dct))
        if target == M.OPAQUE:
            alone = jpeg.encode(want, jpeg.JpegOptions.builder(w, h).color_type(ColorType(int(dct))).quality(80).build())
        else:
            alone = png.encode(want, png.PngOptions.builder(w, h).color_type(ColorType(int(dct))).preset(0).build())
        assert got[i] == alone, "file %d" % i
