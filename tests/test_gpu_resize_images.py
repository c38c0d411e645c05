"""GPU parity of the resize images entries (pixo_hip_resize_images*, the images kernels of resize.hip): N sources of individual
sizes and colour types to N images of individual sizes, anywhere in one block, one flat launch per pass and pixel size.
Image i must be byte for byte what the single entry writes for (source i -> destination i) — which
tests/golden/resize_cases.json pins to the reference's wasm build and resize_reach_cases.json to the model — so every check
here is exact; a failure names the image and the first differing index.  Both blocks are filled with 0xA5 first: guard bands
of 64 bytes and every gap between destinations must stay untouched, and so must the sources.  No test here provokes a
fault; nothing starts a child process.  -m gpu."""
import functools

import numpy as np
import pytest

import resize_cases as RC
import resize_model as M
import resize_reach_cases as RR
from pixo_amd import ColorType, decode, jpeg, png, resize
from test_gpu_resize import device_resize, torch

pytestmark = pytest.mark.gpu

NEAREST, BILINEAR, LANCZOS3 = 0, 1, 2
ALGOS = (NEAREST, BILINEAR, LANCZOS3)
ALGO_BIT = {NEAREST: resize.ROUTE_RESIZE_NEAREST, BILINEAR: resize.ROUTE_RESIZE_BILINEAR, LANCZOS3: resize.ROUTE_RESIZE_LANCZOS3}
GUARD = 64
FILL = 0xA5
SRC_SIZES = [(37, 23), (64, 41), (1, 1), (5, 300), (300, 5), (64, 41), (129, 7), (2200, 2)]
DST_SIZES = [(17, 13), (64, 41), (1, 1), (3, 3), (257, 5), (65, 9), (300, 6), (64, 2)]


def case_of(w, h, dw, dh, ct, algo):
    return dict(name="%s_%dx%d_to_%dx%d_c%d" % (RC.ALGO_NAMES[algo], w, h, dw, dh, ct), sw=w, sh=h, dw=dw, dh=dh, color_type=ct, algorithm=algo)


def same(got, want, what):
    diff = RC.first_difference(got, want)
    assert diff is None, "%s: %s" % (what, diff)


def lay_out(sizes, cts, layout):
    """-> [(width, height, colour type, offset)], end: `packed` (no padding: an image of 4 * k + 1 .. 3 bytes puts the next one
    off a dword), `fit` (every start a multiple of 16, as fit_images lays out), `descending` (image 0 last, 5 bytes between two)"""
    lens = [w * h * RC.BPP[ct] for (w, h), ct in zip(sizes, cts)]
    offsets, at = [], 0
    for n in (lens[::-1] if layout == "descending" else lens):
        offsets.append(at)
        at = {"packed": at + n, "fit": (at + n + 15) // 16 * 16, "descending": at + n + 5}[layout]
    if layout == "descending":
        offsets = offsets[::-1]
    end = max(o + n for o, n in zip(offsets, lens))
    return [(w, h, ct, o) for (w, h), ct, o in zip(sizes, cts, offsets)], end


class Blocks:
    """The source block and the destination block on the device, each with a guard band on both sides and filled with 0xA5
    first; `shift` moves a block's first byte off its aligned base"""

    def __init__(self, srcs, dst_records, dst_end, src_layout="fit", src_shift=0, dst_shift=0):
        t = torch()
        self.src_records, src_end = lay_out([(w, h) for _, w, h, _ in srcs], [ct for _, _, _, ct in srcs], src_layout)
        self.dst_records, self.dst_end = dst_records, dst_end
        host = np.full(src_shift + GUARD + src_end + GUARD, FILL, np.uint8)
        for (px, _, _, _), (_, _, _, at) in zip(srcs, self.src_records):
            host[src_shift + GUARD + at:src_shift + GUARD + at + px.size] = px
        self.src_host = host
        self.src_all = t.from_numpy(host).to("cuda:0")
        self.dst_all = t.full((dst_shift + GUARD + dst_end + GUARD,), FILL, dtype=t.uint8, device="cuda:0")
        assert self.src_all.data_ptr() % 16 == 0 and self.dst_all.data_ptr() % 16 == 0
        self.d_src = self.src_all[src_shift + GUARD:src_shift + GUARD + src_end]
        self.d_dst = self.dst_all[dst_shift + GUARD:dst_shift + GUARD + dst_end]
        self.lead = dst_shift + GUARD
        t.cuda.synchronize()

    def run(self, algo, stream=0):
        resize.resize_images_device(self.d_src, self.src_records, self.d_dst, self.dst_records, algo, stream)

    def images(self, what=""):
        """(after a synchronise) the images as a list of bytes; everything else must be as it was"""
        got = self.dst_all.cpu().numpy()
        written = np.zeros(got.size, bool)
        out = []
        for w, h, ct, at in self.dst_records:
            n = w * h * RC.BPP[ct]
            assert not written[self.lead + at:self.lead + at + n].any(), "the test's own destinations overlap"
            written[self.lead + at:self.lead + at + n] = True
            out.append(got[self.lead + at:self.lead + at + n].tobytes())
        touched = np.flatnonzero(~written & (got != FILL))
        assert touched.size == 0, "%s: byte %d of the destination block (guard band or gap; the block starts at %d) was written" % (what, touched[0], self.lead)
        assert np.array_equal(self.src_all.cpu().numpy(), self.src_host), "%s: the source block was written" % what
        return out


def images_device(srcs, dsts, algo, layout="fit", src_layout="fit", src_shift=0, dst_shift=0, what=""):
    """srcs: [(pixels, w, h, colour type)], dsts: [(dw, dh)] -> the images as a list of bytes, through ONE resize_images_device call"""
    records, end = lay_out(dsts, [ct for _, _, _, ct in srcs], layout)
    b = Blocks(srcs, records, end, src_layout, src_shift, dst_shift)
    b.run(algo)
    torch().cuda.synchronize()
    return b.images(what)


@functools.lru_cache(maxsize=None)
def ragged(rotation):
    """The ragged set with the colour type cycling 0..3 over the images, the cycle rotated"""
    return tuple((RC.make_input(dict(sw=w, sh=h, color_type=(i + rotation) % 4, gen="lcg", seed=700 + i)), w, h, (i + rotation) % 4)
                 for i, (w, h) in enumerate(SRC_SIZES))


@functools.lru_cache(maxsize=None)
def singles(rotation, algo):
    """What the single entry writes for every pair of the ragged set (computed once, shared, never changed)"""
    return tuple(device_resize(case_of(w, h, dw, dh, ct, algo), px) for (px, w, h, ct), (dw, dh) in zip(ragged(rotation), DST_SIZES))


def check_ragged(got, rotation, algo, what):
    want = singles(rotation, algo)
    assert len(got) == len(want)
    for i in range(len(want)):
        same(got[i], want[i], "%s, %s rotation %d, image %d against the single entry" % (what, RC.ALGO_NAMES[algo], rotation, i))


# ---- 1. the golden vectors: one call per algorithm, mixed colour types, individual destinations --------------------------------
SMALL = [c for c in RC.ok_cases() if c["len"] <= 4_000_000]


@pytest.mark.parametrize("algo", ALGOS)
def test_golden_cases_of_one_algorithm_in_one_call(algo):
    cs = [c for c in SMALL if c["algorithm"] == algo]
    assert len(cs) > 8 and len({c["color_type"] for c in cs}) == 4 and len({(c["dw"], c["dh"]) for c in cs}) > 4
    got = images_device([(RC.make_input(c), c["sw"], c["sh"], c["color_type"]) for c in cs], [(c["dw"], c["dh"]) for c in cs], algo,
                        what=RC.ALGO_NAMES[algo])
    for c, img in zip(cs, got):
        RC.check(c, img)


REACH = [c for c in RR.CASES if c["name"] != RR.MAKER_ONLY]


@pytest.mark.parametrize("c", REACH, ids=[c["name"] for c in REACH])
def test_reach_case_and_a_small_companion_in_one_launch(c):
    """The LDS / direct threshold, the row-stride loops and the cap on an image's rows of tiles in the images kernels; the
    companion's few tiles share the launch, in front of the case's and behind them"""
    ct, algo = c["color_type"], c["algorithm"]
    small = RC.make_input(dict(sw=3, sh=3, color_type=ct, gen="lcg", seed=77))
    srcs, dsts = [(RC.make_input(c), c["sw"], c["sh"], ct), (small, 3, 3, ct)], [(c["dw"], c["dh"]), (5, 4)]
    want = device_resize(case_of(3, 3, 5, 4, ct, algo), small)
    for order in (0, 1):
        got = images_device(srcs[::-1] if order else srcs, dsts[::-1] if order else dsts, algo, what=c["name"])
        got = got[::-1] if order else got
        RR.check(c, got[0], "as image %d of two" % order)
        same(got[1], want, "%s: the companion as image %d" % (c["name"], 1 - order))


# ---- 2. the ragged set against the single entry and the model --------------------------------------------------------------------
@pytest.mark.parametrize("rotation", range(4))
@pytest.mark.parametrize("algo", ALGOS)
def test_ragged_set_equals_single_entry_and_model(algo, rotation):
    srcs = ragged(rotation)
    records, _ = lay_out(DST_SIZES, [ct for _, _, _, ct in srcs], "fit")
    plan = resize.resize_images_plan([(w, h, ct, 0) for _, w, h, ct in srcs], records, algo)
    assert plan["sub_first"] == [0, 8] and plan["launches_first"] == 4 and plan["launches_second"] == (1 if algo == LANCZOS3 else 0)
    if algo == LANCZOS3:
        # 2200 source pixels under one tile: 2200 * bpp + 8 bytes fit the 8192-byte segment up to 3 bytes a pixel, not at 4 —
        # over the rotations the last image is staged three times and direct once, beside staged images of its launch
        assert plan["use_lds"] == [True] * 7 + [srcs[7][3] < 3]
        assert plan["tiles_first"][5] == 2 * 11 and plan["tiles_second"][6] == (2 if srcs[6][3] == 3 else 1) * 6
    else:
        assert plan["tiles_first"][4] == 2 * 2
    got = images_device(list(srcs), DST_SIZES, algo, what="%s rotation %d" % (RC.ALGO_NAMES[algo], rotation))
    check_ragged(got, rotation, algo, "one call")
    for i, ((px, w, h, ct), (dw, dh)) in enumerate(zip(srcs, DST_SIZES)):
        same(got[i], M.resize(px, w, h, dw, dh, RC.BPP[ct], algo), "%s, image %d against the model" % (case_of(w, h, dw, dh, ct, algo)["name"], i))


# ---- 3. layouts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_layouts_and_unaligned_blocks(algo):
    rotation = 3  # the 3x3 destination is RGB: 27 bytes, the next image starts off a dword when packed
    srcs = list(ragged(rotation))
    assert srcs[3][3] == 2
    for layout in ("packed", "fit", "descending"):
        records, _ = lay_out(DST_SIZES, [ct for _, _, _, ct in srcs], layout)
        if layout == "packed":
            assert records[4][3] - records[3][3] == 27 and records[4][3] % 4 != records[3][3] % 4
        if layout == "descending":
            assert all(a[3] > b[3] for a, b in zip(records, records[1:]))
        check_ragged(images_device(srcs, DST_SIZES, algo, layout=layout, what=layout), rotation, algo, layout)
    # the 16-byte layout as fit_images itself makes it
    fitted, total = resize.fit_images([(w, h, ct, 0) for _, w, h, ct in srcs], 40, 40)
    assert [r[3] for r in fitted] == [r[3] for r in lay_out([(w, h) for w, h, _, _ in fitted], [int(ct) for _, _, ct, _ in fitted], "fit")[0]]
    b = Blocks(srcs, fitted, total)
    b.run(algo)
    torch().cuda.synchronize()
    for i, (img, (px, w, h, ct), (dw, dh, _, _)) in enumerate(zip(b.images("fit_images"), srcs, fitted)):
        same(img, device_resize(case_of(w, h, dw, dh, ct, algo), px), "fitted into 40x40, %s, image %d" % (RC.ALGO_NAMES[algo], i))
    # packed sources too, and both blocks at every offset from an aligned base
    for so, do in ((0, 0), (1, 3), (2, 1), (3, 2)):
        got = images_device(srcs, DST_SIZES, algo, layout="packed", src_layout="packed", src_shift=so, dst_shift=do, what="shifts %d %d" % (so, do))
        check_ragged(got, rotation, algo, "sources +%d, destinations +%d" % (so, do))


# ---- 4. switches and streams --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_row_cap_and_sub_batches_equal_the_uncut_call(algo):
    rotation = 1
    srcs = list(ragged(rotation))
    src_records = [(w, h, ct, 0) for _, w, h, ct in srcs]
    dst_records, _ = lay_out(DST_SIZES, [ct for _, _, _, ct in srcs], "fit")
    uncut = images_device(srcs, DST_SIZES, algo)
    check_ragged(uncut, rotation, algo, "uncut")
    try:
        for rows in (1, 2):  # the row-stride loops: every image has one or two rows of tiles
            jpeg.debug_configure("resize_images_rows=%d" % rows)
            plan = resize.resize_images_plan(src_records, dst_records, algo)
            assert max(t // -(-dw // (64 if algo == LANCZOS3 else 256)) for t, (dw, _) in zip(plan["tiles_first"], DST_SIZES)) == rows
            got = images_device(srcs, DST_SIZES, algo, what="rows %d" % rows)
            for i in range(len(srcs)):
                same(got[i], uncut[i], "%s, resize_images_rows=%d, image %d" % (RC.ALGO_NAMES[algo], rows, i))
        for limit, subs in ((20000, 2), (1, len(srcs))):
            jpeg.debug_configure("resize_batch_bytes=%d" % limit)
            plan = resize.resize_images_plan(src_records, dst_records, algo)
            assert len(plan["sub_first"]) - 1 == (subs if algo == LANCZOS3 else 1)
            jpeg.debug_routes(clear=True)
            got = images_device(srcs, DST_SIZES, algo, what="limit %d" % limit)
            bits = jpeg.debug_routes(clear=True)
            assert bool(bits & jpeg.ROUTE_SUB_BATCHES) == (algo == LANCZOS3)
            for i in range(len(srcs)):
                same(got[i], uncut[i], "%s, resize_batch_bytes=%d, image %d" % (RC.ALGO_NAMES[algo], limit, i))
    finally:
        jpeg.debug_configure(None)


def test_two_calls_back_to_back_on_one_stream():
    """Call A, then call B with other tables and records, no host wait between them: B's replace A's in the same staging memory"""
    t = torch()
    s = t.cuda.Stream()
    for algo in (LANCZOS3, BILINEAR):
        a_src, b_src = list(ragged(0)), list(ragged(2))[::-1][:5]
        a_dst, b_dst = DST_SIZES, [(9, 31), (40, 3), (64, 2), (1, 7), (33, 33)]
        with t.cuda.stream(s):
            a = Blocks(a_src, *lay_out(a_dst, [ct for _, _, _, ct in a_src], "fit"))
            b = Blocks(b_src, *lay_out(b_dst, [ct for _, _, _, ct in b_src], "packed"))
        with jpeg.producer_stream(s.cuda_stream):
            for _ in range(2):
                a.run(algo, s.cuda_stream)
                b.run(algo, s.cuda_stream)
        t.cuda.synchronize()
        check_ragged(a.images("call A"), 0, algo, "call A")
        for i, (img, (px, w, h, ct), (dw, dh)) in enumerate(zip(b.images("call B"), b_src, b_dst)):
            same(img, device_resize(case_of(w, h, dw, dh, ct, algo), px), "%s call B, image %d" % (RC.ALGO_NAMES[algo], i))


def test_host_entry_equals_the_device_entry():
    srcs = list(ragged(2))
    src_records, src_end = lay_out([(w, h) for _, w, h, _ in srcs], [ct for _, _, _, ct in srcs], "fit")
    dst_records, _ = lay_out(DST_SIZES, [ct for _, _, _, ct in srcs], "descending")
    block = np.zeros(src_end, np.uint8)
    for (px, _, _, _), (_, _, _, at) in zip(srcs, src_records):
        block[at:at + px.size] = px
    for algo in ALGOS:
        check_ragged(resize.resize_images(block, src_records, dst_records, algo), 2, algo, "host entry")


# ---- 5. the chain: decode batch -> fit -> resize images -> encode images ---------------------------------------------------------
def test_decode_fit_resize_encode_without_leaving_the_device():
    t = torch()
    shapes = [(61, 40, 2), (33, 57, 3), (24, 24, 0), (90, 11, 1), (7, 48, 2)]
    pixels = [RC.make_input(dict(sw=w, sh=h, color_type=ct, gen="lcg", seed=900 + i)) for i, (w, h, ct) in enumerate(shapes)]
    files = [png.encode(px, png.PngOptions.builder(w, h).color_type(ColorType(ct)).preset(0).build()) for px, (w, h, ct) in zip(pixels, shapes)]
    template = png.PngOptions.builder(0, 0).preset(0).build()
    s = t.cuda.current_stream().cuda_stream
    views = decode.decode_png_batch_device(files)
    assert [(v.shape[1], v.shape[0], int(ct)) for v, ct in views] == shapes
    fitted, total = resize.fit_images(views, 24, 24)
    d_dst = t.full((total,), FILL, dtype=t.uint8, device="cuda:0")
    resize.resize_images_device(None, views, d_dst, fitted, LANCZOS3, s)  # (the views carry their block with them)
    out = png.encode_images_device(d_dst, fitted, template)
    assert [(w, h) for w, h, _, _ in fitted] == [(24, 16), (14, 24), (24, 24), (24, 3), (4, 24)]
    for i, (file_bytes, px, (w, h, ct), (dw, dh, dct, _)) in enumerate(zip(out, pixels, shapes, fitted)):
        image = decode.decode_png(file_bytes)
        assert (image.width, image.height, int(image.color_type)) == (dw, dh, ct) and int(dct) == ct, "file %d" % i
        same(bytes(image.pixels), M.resize(px, w, h, dw, dh, RC.BPP[ct], LANCZOS3), "file %d: %dx%d c%d -> %dx%d against the model" % (i, w, h, ct, dw, dh))


# ---- 6. routes ------------------------------------------------------------------------------------------------------------------------
def test_routes_are_noted():
    srcs = list(ragged(0))
    for algo in ALGOS:
        jpeg.debug_routes(clear=True)
        images_device(srcs, DST_SIZES, algo)
        bits = jpeg.debug_routes(clear=True)
        assert bits & resize.ROUTE_RESIZE_IMAGES and not bits & resize.ROUTE_RESIZE_BATCH and not bits & jpeg.ROUTE_SUB_BATCHES
        assert bits & sum(ALGO_BIT.values()) == ALGO_BIT[algo]
    try:
        jpeg.debug_configure("resize_batch_bytes=4096")
        images_device(srcs, DST_SIZES, LANCZOS3)
        bits = jpeg.debug_routes(clear=True)
        assert bits & resize.ROUTE_RESIZE_IMAGES and bits & jpeg.ROUTE_SUB_BATCHES and bits & resize.ROUTE_RESIZE_LANCZOS3
    finally:
        jpeg.debug_configure(None)
    images_device(srcs, DST_SIZES, LANCZOS3)
    assert not jpeg.debug_routes(clear=True) & jpeg.ROUTE_SUB_BATCHES
