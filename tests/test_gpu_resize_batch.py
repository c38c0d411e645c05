"""GPU parity of the resize batch entries (pixo_hip_resize_batch*, the batch kernels of resize.hip): N sources of individual
sizes to N images of one size, back to back.  Image i must be byte for byte what the single entry writes for source i — which
tests/golden/resize_cases.json pins to the reference's wasm build and resize_reach_cases.json to the model — so every check
here is exact; a failure names the image and the first differing index.  No test here provokes a fault; nothing starts a
child process.  -m gpu."""
import functools
import threading

import numpy as np
import pytest

import resize_cases as RC
import resize_model as M
import resize_reach_cases as RR
from pixo_amd import ColorType, _lib, jpeg, png, resize
from test_gpu_resize import device_resize, on_device, options, torch

pytestmark = pytest.mark.gpu

NEAREST, BILINEAR, LANCZOS3 = 0, 1, 2
ALGO_BIT = {NEAREST: resize.ROUTE_RESIZE_NEAREST, BILINEAR: resize.ROUTE_RESIZE_BILINEAR, LANCZOS3: resize.ROUTE_RESIZE_LANCZOS3}
GUARD = 64
RAGGED = [(37, 23), (64, 41), (1, 1), (5, 300), (300, 5), (64, 41), (129, 7)]
DESTS = [(17, 13), (64, 41), (3, 3)]


def batch_device(srcs, dw, dh, ct, algo, stream=0, src_offset=0, dst_offset=0, what=""):
    """srcs: [(pixels, w, h)] -> the images as a list of bytes, through resize_batch_device with a guard band of 0xA5 on both
    sides of the block"""
    t = torch()
    each = dw * dh * RC.BPP[ct]
    lead = GUARD + dst_offset
    d_srcs = [(on_device(px, src_offset), w, h) for px, w, h in srcs]
    d_all = t.full((lead + len(srcs) * each + GUARD,), 0xA5, dtype=t.uint8, device="cuda:0")
    t.cuda.synchronize()
    resize.resize_batch_device(d_srcs, dw, dh, ct, algo, d_all[lead:lead + len(srcs) * each], stream)
    t.cuda.synchronize()
    got = d_all.cpu().numpy()
    assert (got[:lead] == 0xA5).all() and (got[lead + len(srcs) * each:] == 0xA5).all(), "%s: bytes outside the block were written" % what
    return [got[lead + i * each:lead + (i + 1) * each].tobytes() for i in range(len(srcs))]


def case_of(w, h, dw, dh, ct, algo):
    return dict(name="%s_%dx%d_to_%dx%d_c%d" % (RC.ALGO_NAMES[algo], w, h, dw, dh, ct), sw=w, sh=h, dw=dw, dh=dh, color_type=ct, algorithm=algo)


def same(got, want, what):
    diff = RC.first_difference(got, want)
    assert diff is None, "%s: %s" % (what, diff)


@functools.lru_cache(maxsize=None)
def ragged_pixels(ct):
    return tuple((RC.make_input(dict(sw=w, sh=h, color_type=ct, gen="lcg", seed=500 + i)), w, h) for i, (w, h) in enumerate(RAGGED))


@functools.lru_cache(maxsize=None)
def singles(ct, algo, dw, dh):
    """What the single entry writes for every ragged source (computed once, shared)"""
    return tuple(device_resize(case_of(w, h, dw, dh, ct, algo), px) for px, w, h in ragged_pixels(ct))


# ---- 1. the golden vectors, as a batch of one and of three ------------------------------------------------------------------------
SMALL = [c for c in RC.ok_cases() if c["len"] <= 4_000_000]


@pytest.mark.parametrize("c", SMALL, ids=[c["name"] for c in SMALL])
def test_golden_as_batch_of_one_and_of_three(c):
    px = RC.make_input(c)
    for n in (1, 3):
        got = batch_device([(px, c["sw"], c["sh"])] * n, c["dw"], c["dh"], c["color_type"], c["algorithm"], what=c["name"])
        for img in got:
            RC.check(c, img)


def test_golden_cases_of_one_destination_as_one_mixed_batch():
    """Golden cases that share destination, colour type and algorithm run as one batch of their different sources."""
    groups = {}
    for c in SMALL:
        groups.setdefault((c["dw"], c["dh"], c["color_type"], c["algorithm"]), []).append(c)
    for (dw, dh, ct, algo), cs in groups.items():
        if len(cs) > 1:
            got = batch_device([(RC.make_input(c), c["sw"], c["sh"]) for c in cs], dw, dh, ct, algo)
            for c, img in zip(cs, got):
                RC.check(c, img)


# ---- 2. the reach vectors, each beside a 3x3 companion in the same launch -----------------------------------------------------
REACH = [c for c in RR.CASES if c["name"] != RR.MAKER_ONLY]


@pytest.mark.parametrize("c", REACH, ids=[c["name"] for c in REACH])
def test_reach_case_and_a_small_companion_in_one_launch(c):
    """The LDS / direct threshold, the row-stride loops and the grid.y cap in the batch kernels; the companion's few rows and
    its LDS staging share the launch (grid.y is sized for the case)."""
    ct, algo, dw, dh = c["color_type"], c["algorithm"], c["dw"], c["dh"]
    small = RC.make_input(dict(sw=3, sh=3, color_type=ct, gen="lcg", seed=77))
    srcs = [(RC.make_input(c), c["sw"], c["sh"]), (small, 3, 3)]
    for order in (0, 1):
        got = batch_device(srcs[::-1] if order else srcs, dw, dh, ct, algo, what=c["name"])
        got = got[::-1] if order else got
        RR.check(c, got[0], "as image %d of two" % order)
        same(got[1], device_resize(case_of(3, 3, dw, dh, ct, algo), small), "%s: the companion as image %d" % (c["name"], 1 - order))


# ---- 3. ragged batches against the single entry and the model -------------------------------------------------------------------
@pytest.mark.parametrize("ct", range(4))
@pytest.mark.parametrize("algo", (NEAREST, BILINEAR, LANCZOS3))
def test_ragged_batch_equals_single_entry_and_model(algo, ct):
    """(3, 3) at 3 bytes a pixel gives 27-byte images: images 1, 2, ... start off a dword"""
    srcs = ragged_pixels(ct)
    for dw, dh in DESTS:
        got = batch_device(list(srcs), dw, dh, ct, algo, what="%s c%d -> %dx%d" % (RC.ALGO_NAMES[algo], ct, dw, dh))
        want = singles(ct, algo, dw, dh)
        for i, (px, w, h) in enumerate(srcs):
            what = "%s, image %d" % (case_of(w, h, dw, dh, ct, algo)["name"], i)
            same(got[i], want[i], what + " against the single entry")
            same(got[i], M.resize(px, w, h, dw, dh, RC.BPP[ct], algo), what + " against the model")


# ---- 4. caller pointers off a dword -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", (NEAREST, BILINEAR, LANCZOS3))
def test_unaligned_sources_and_destination(algo):
    for ct, (dw, dh) in ((2, (17, 13)), (0, (3, 3)), (3, (64, 41)), (1, (17, 13))):
        want = singles(ct, algo, dw, dh)
        for so, do in ((1, 3), (2, 1), (3, 2)):
            got = batch_device(list(ragged_pixels(ct)), dw, dh, ct, algo, src_offset=so, dst_offset=do)
            for i in range(len(RAGGED)):
                same(got[i], want[i], "%s c%d -> %dx%d, image %d, sources +%d, destination +%d" % (RC.ALGO_NAMES[algo], ct, dw, dh, i, so, do))


# ---- 5. sub-batches ---------------------------------------------------------------------------------------------------------------------
def test_sub_batches_equal_the_uncut_call_and_routes_are_noted():
    ct, (dw, dh) = 2, (17, 13)
    srcs = list(ragged_pixels(ct))[:2] + list(ragged_pixels(ct))[3:]  # six images
    sizes = [(w, h) for _, w, h in srcs]
    jpeg.debug_routes(clear=True)
    uncut = batch_device(srcs, dw, dh, ct, LANCZOS3)
    bits = jpeg.debug_routes(clear=True)
    assert bits & resize.ROUTE_RESIZE_BATCH and bits & resize.ROUTE_RESIZE_LANCZOS3 and not bits & jpeg.ROUTE_SUB_BATCHES
    try:
        for limit in (4096, 1):
            jpeg.debug_configure("resize_batch_bytes=%d" % limit)
            assert len(resize.resize_batch_plan(sizes, dw, dh, ct, LANCZOS3)["sub_first"]) - 1 >= 3
            cut = batch_device(srcs, dw, dh, ct, LANCZOS3)
            bits = jpeg.debug_routes(clear=True)
            assert bits & jpeg.ROUTE_SUB_BATCHES and bits & resize.ROUTE_RESIZE_BATCH and bits & resize.ROUTE_RESIZE_LANCZOS3
            for i in range(len(srcs)):
                same(cut[i], uncut[i], "limit %d, image %d" % (limit, i))
        # nearest and bilinear have no intermediate: never cut
        for algo in (NEAREST, BILINEAR):
            batch_device(srcs, dw, dh, ct, algo)
            bits = jpeg.debug_routes(clear=True)
            assert bits & resize.ROUTE_RESIZE_BATCH and not bits & jpeg.ROUTE_SUB_BATCHES
            assert bits & sum(ALGO_BIT.values()) == ALGO_BIT[algo]
    finally:
        jpeg.debug_configure(None)
    assert resize.resize_batch_plan(sizes, dw, dh, ct, LANCZOS3)["sub_first"] == [0, len(srcs)]
    want = [s for k, s in enumerate(singles(ct, LANCZOS3, dw, dh)) if k != 2]
    for i in range(len(srcs)):
        same(uncut[i], want[i], "image %d against the single entry" % i)


# ---- 6. calls back to back ---------------------------------------------------------------------------------------------------------------
def test_two_batches_back_to_back_on_one_stream():
    """Batch A, then batch B of other sizes, one synchronise: B's tables and items replace A's in the same staging memory"""
    t = torch()
    ct = 2
    a, b = list(ragged_pixels(ct)), [s for s in ragged_pixels(ct)][::-1][:5]
    (adw, adh), (bdw, bdh) = (17, 13), (64, 41)
    s = t.cuda.Stream()
    for algo in (LANCZOS3, BILINEAR):
        want_a, want_b = singles(ct, algo, adw, adh), singles(ct, algo, bdw, bdh)[::-1][:5]
        with t.cuda.stream(s):
            da = [(t.from_numpy(px).to("cuda:0"), w, h) for px, w, h in a]
            db = [(t.from_numpy(px).to("cuda:0"), w, h) for px, w, h in b]
            oa = t.full((len(a) * adw * adh * 3,), 0xA5, dtype=t.uint8, device="cuda:0")
            ob = t.full((len(b) * bdw * bdh * 3,), 0xA5, dtype=t.uint8, device="cuda:0")
        with jpeg.producer_stream(s.cuda_stream):
            for rnd in range(2):
                resize.resize_batch_device(da, adw, adh, ct, algo, oa, s.cuda_stream)
                resize.resize_batch_device(db, bdw, bdh, ct, algo, ob, s.cuda_stream)
        t.cuda.synchronize()
        ga, gb = oa.cpu().numpy().tobytes(), ob.cpu().numpy().tobytes()
        for i in range(len(a)):
            same(ga[i * adw * adh * 3:(i + 1) * adw * adh * 3], want_a[i], "%s batch A, image %d" % (RC.ALGO_NAMES[algo], i))
        for i in range(len(b)):
            same(gb[i * bdw * bdh * 3:(i + 1) * bdw * bdh * 3], want_b[i], "%s batch B, image %d" % (RC.ALGO_NAMES[algo], i))


def test_single_batch_single_with_a_trim_between():
    """The batch has buffers of its own: the single entry's cached tables still serve behind it"""
    c = next(c for c in SMALL if c["name"].startswith("lanczos3_64x48_to_17x13_c2"))
    px = RC.make_input(c)
    ct, dw, dh = 2, 17, 13
    want = singles(ct, LANCZOS3, dw, dh)
    for trim_at in (None, 1, 2):
        for step in range(3):
            if trim_at == step:
                assert _lib.load().pixo_hip_trim() == 0
            if step == 1:
                got = batch_device(list(ragged_pixels(ct)), dw, dh, ct, LANCZOS3)
                for i in range(len(RAGGED)):
                    same(got[i], want[i], "trim at %s, image %d" % (trim_at, i))
            else:
                RC.check(c, device_resize(c, px))
    assert _lib.load().pixo_hip_trim() == 0


# ---- 7. into the batch encoders on one stream ---------------------------------------------------------------------------------------
def test_pipeline_into_the_batch_encoders_on_one_stream():
    t = torch()
    ct, (dw, dh) = 2, (64, 41)
    srcs = ragged_pixels(ct)
    n = len(srcs)
    each = dw * dh * 3
    po = png.PngOptions.builder(dw, dh).color_type(ColorType.Rgb).preset(1).build()
    jo = jpeg.JpegOptions.builder(dw, dh).color_type(ColorType.Rgb).quality(80).subsampling(jpeg.Subsampling.S420).build()
    s = t.cuda.Stream()
    for algo in (BILINEAR, LANCZOS3):
        singly = t.from_numpy(np.frombuffer(b"".join(singles(ct, algo, dw, dh)), np.uint8).copy()).to("cuda:0")
        t.cuda.synchronize()
        want_png, want_jpeg = png.encode_batch_device(singly, po, n), jpeg.encode_batch_device(singly, jo, n)
        with t.cuda.stream(s):
            d_srcs = [(t.from_numpy(px).to("cuda:0"), w, h) for px, w, h in srcs]
            d_dst = t.full((n * each,), 0xA5, dtype=t.uint8, device="cuda:0")
        with jpeg.producer_stream(s.cuda_stream):
            resize.resize_batch_device(d_srcs, dw, dh, ct, algo, d_dst, s.cuda_stream)
            got_png = png.encode_batch_device(d_dst, po, n)
            resize.resize_batch_device(d_srcs, dw, dh, ct, algo, d_dst, s.cuda_stream)
            got_jpeg = jpeg.encode_batch_device(d_dst, jo, n)
        t.cuda.synchronize()
        assert got_png == want_png, RC.ALGO_NAMES[algo]
        assert got_jpeg == want_jpeg, RC.ALGO_NAMES[algo]


# ---- 8. host pixels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", (NEAREST, BILINEAR, LANCZOS3))
def test_host_entry_equals_per_image_resize(algo):
    for ct, (dw, dh) in ((2, (3, 3)), (3, (17, 13)), (0, (64, 41))):
        srcs = ragged_pixels(ct)
        got = resize.resize_batch(list(srcs), dw, dh, ct, algo)
        assert len(got) == len(srcs)
        for i, (px, w, h) in enumerate(srcs):
            same(got[i], resize.resize(px, options(case_of(w, h, dw, dh, ct, algo))), "%s c%d, image %d" % (RC.ALGO_NAMES[algo], ct, i))


# ---- 9. two calling threads -----------------------------------------------------------------------------------------------------------
def test_two_calling_threads_each_with_its_own_batches():
    want = {(ct, algo): singles(ct, algo, 17, 13) for ct in (2, 3) for algo in (BILINEAR, LANCZOS3)}
    errors = []

    def work(k):
        try:
            ct = 2 + k
            for rep in range(3):
                for algo in (LANCZOS3, BILINEAR):
                    srcs = list(ragged_pixels(ct))[k:] if rep % 2 else list(ragged_pixels(ct))
                    first = k if rep % 2 else 0
                    got = resize.resize_batch(srcs, 17, 13, ct, algo) if rep == 2 else batch_device(srcs, 17, 13, ct, algo)
                    for i, img in enumerate(got):
                        same(img, want[ct, algo][first + i], "thread %d, round %d, image %d" % (k, rep, i))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert not any(th.is_alive() for th in threads), "a calling thread did not finish"
    assert not errors, errors[:3]
