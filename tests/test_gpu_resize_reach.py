"""GPU parity of resize on the paths tests/resize_reach_cases.py names (each claim is held without a GPU by
tests/test_resize_reach_cpu.py): the horizontal Lanczos3 pass without LDS staging and with the staging exactly full, a second
round of each kernel's row-stride loop, sides of 2^24, and the call sequences that make one context change between those
paths with its tables cached.  Byte for byte against the recorded output; a failure names the case and the first differing
index.  No test here provokes a fault; nothing starts a child process.  -m gpu."""
import functools

import numpy as np
import pytest

import resize_cases as RC
import resize_model as M
import resize_reach_cases as RR
from pixo_amd import _lib, resize
from test_gpu_resize import device_resize, options, torch

pytestmark = pytest.mark.gpu

IDS = [c["name"] for c in RR.CASES]
DIRECT_RGBA = "lanczos3_2047x5_to_1x3_c3"  # one pixel past the LDS capacity; the shape of every call sequence below


@functools.lru_cache(maxsize=None)
def _input(name):
    px = RC.make_input(RR.by_name(name))
    return px


def pixels(c):
    return _input(c["name"])


def both_entries(c, what=""):
    """host pixels through resize(), device pixels through resize_device(), in that order in this thread's context"""
    RR.check(c, resize.resize(pixels(c), options(c)), ("resize " + what).strip())
    RR.check(c, device_resize(c, pixels(c)), ("resize_device " + what).strip())


@pytest.mark.parametrize("c", RR.CASES, ids=IDS)
def test_recorded_bytes_through_resize(c):
    RR.check(c, resize.resize(pixels(c), options(c)))


@pytest.mark.parametrize("c", RR.CASES, ids=IDS)
def test_recorded_bytes_through_resize_device(c):
    RR.check(c, device_resize(c, pixels(c)))


@pytest.mark.parametrize("c", RR.A_CASES, ids=[c["name"] for c in RR.A_CASES])
def test_threshold_and_direct_cases_at_unaligned_pointers(c):
    """A source 3 bytes past a dword puts three bytes in front of the staged segment: with the exactly full cases that is the
    largest the staging ever gets (8188 of 8192 bytes).  The direct branch reads bytes and must not care."""
    for so, do in ((3, 1), (1, 3)):
        RR.check(c, device_resize(c, pixels(c), src_offset=so, dst_offset=do), "source +%d, destination +%d" % (so, do))


def test_cached_tables_serve_every_pixel_size():
    """One shape, so the tables and the span stay cached; the pixel size alone moves the launch between LDS staging and
    direct loads: on, off, on, on, off."""
    seq = [RR.by_name("lanczos3_2047x5_to_1x3_c%d" % ct) for ct in (0, 3, 0, 2, 3)]
    assert [c["use_lds"] for c in seq] == [True, False, True, True, False]
    assert len({(c["sw"], c["dw"], c["sh"], c["dh"]) for c in seq}) == 1
    for k, c in enumerate(seq):
        both_entries(c, "step %d" % k)


def test_algorithm_changes_on_one_shape():
    for k, name in enumerate((DIRECT_RGBA, "nearest_2047x5_to_1x3_c3", DIRECT_RGBA)):
        both_entries(RR.by_name(name), "step %d" % k)


def test_swapped_axes_are_another_shape():
    """(sw, dw, sh, dh) = (2047, 1, 5, 3) and (5, 3, 2047, 1): the same four numbers, other tables and another span"""
    a, b = RR.by_name(DIRECT_RGBA), RR.by_name("lanczos3_5x2047_to_3x1_c3")
    assert sorted((a["sw"], a["dw"], a["sh"], a["dh"])) == sorted((b["sw"], b["dw"], b["sh"], b["dh"]))
    for k, c in enumerate((a, b, a, b)):
        both_entries(c, "step %d" % k)


def test_one_dimension_changes_at_a_time():
    """The tables belong to all four of (src_w, dst_w, src_h, dst_h): each neighbour differs from the base shape in exactly
    one of them (the pixel size is free: the tables do not depend on it), and the base comes back after each."""
    base = RR.by_name(DIRECT_RGBA)
    key = lambda c: (c["sw"], c["dw"], c["sh"], c["dh"])  # noqa: E731
    for k, other in enumerate(("lanczos3_2728x5_to_1x3_c2", "lanczos3_2047x5_to_2x3_c3", "lanczos3_2047x6_to_1x3_c3", "lanczos3_2047x5_to_1x2_c3")):
        c = RR.by_name(other)
        assert [a != b for a, b in zip(key(c), key(base))] == [j == k for j in range(4)]
        both_entries(base, "before the neighbour in dimension %d" % k)
        both_entries(c, "the neighbour in dimension %d" % k)
    both_entries(base, "at the end")


@pytest.mark.parametrize("name", ["lanczos3_20000x6_to_100x5_c2", "lanczos3_2046x5_to_1x3_c3"], ids=["direct", "lds"])
def test_two_streams_share_one_context(name):
    """Two jobs of one shape on two non-default streams, no host synchronisation between the calls: the second finds the
    tables cached and is ordered behind the first (its upload included) by the context's event alone.  Each job has its own
    pixels and output; the second image is the first reversed, its expected bytes are the model's."""
    t = torch()
    c = RR.by_name(name)
    o = options(c)
    n = o.output_len()
    px = [pixels(c), np.ascontiguousarray(pixels(c)[::-1])]
    assert not np.array_equal(px[0], px[1])
    want1 = M.resize(px[1], c["sw"], c["sh"], c["dw"], c["dh"], RR.bpp(c), c["algorithm"])
    streams = [t.cuda.Stream(), t.cuda.Stream()]
    assert len({0, streams[0].cuda_stream, streams[1].cuda_stream}) == 3
    assert _lib.load().pixo_hip_trim() == 0  # (the first call of the first round uploads the tables on its own stream)
    for rnd in range(3):
        src = [t.from_numpy(p).to("cuda:0") for p in px]
        whole = [t.full((n + 32,), 0xA5, dtype=t.uint8, device="cuda:0") for _ in px]
        order = (0, 1) if rnd % 2 == 0 else (1, 0)
        t.cuda.synchronize()
        for k in order:
            resize.resize_device(src[k], o, whole[k][16:16 + n], streams[k].cuda_stream)
        t.cuda.synchronize()
        for k in order:
            got = whole[k].cpu().numpy()
            what = "round %d, stream %d" % (rnd, k)
            assert (got[:16] == 0xA5).all() and (got[16 + n:] == 0xA5).all(), "%s %s: bytes outside the output were written" % (name, what)
            if k == 0:
                RR.check(c, got[16:16 + n].tobytes(), what)
            else:
                diff = RC.first_difference(got[16:16 + n].tobytes(), want1)
                assert diff is None, "%s %s: %s" % (name, what, diff)


def test_trim_between_two_direct_calls():
    c = RR.by_name("lanczos3_9000x5_to_70x3_c3")
    assert not c["use_lds"]
    both_entries(c, "before the trim")
    assert _lib.load().pixo_hip_trim() == 0
    both_entries(c, "after the trim")
    assert _lib.load().pixo_hip_trim() == 0
    RR.check(c, device_resize(c, pixels(c)), "resize_device first after a trim")
