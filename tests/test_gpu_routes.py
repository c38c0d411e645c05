"""Deterministic route matrix: named call histories, each checked byte for byte against the oracle AND for the route bits
it must have taken (include/pixo_hip.h pixo_hip_debug_routes).  Includes the grow pairs of the seed-955 class: on a freshly
trimmed thread a small call, then a call that grows the context's grow-only buffers on a route that has already handed
pointers derived from them to a kernel."""
import numpy as np
import pytest

import oracle_lib as O
import route_runner as RR
from pixo_amd import jpeg

pytestmark = pytest.mark.gpu


def case(w, h, entry="encode", ct=2, ss=1, q=80, content="noise", cseed=5, opt=False, prog=False, trellis=False,
         restart=None, **kw):
    d = dict(kind="jpeg", entry=entry, w=w, h=h, ct=ct, ss=ss, q=q, content=content, cseed=cseed, opt=opt, prog=prog,
             trellis=trellis, restart=restart, trim=False, seed=0, i=0)
    d.update(kw)
    return d


def run(d):
    """Runs case d, checks it against the oracle and returns the route bits of the call."""
    import random_cases as R
    want = R.expected(d, O)
    jpeg.debug_routes(clear=True)
    got = RR.run_jpeg(d, want)
    bits = jpeg.debug_routes(clear=True)
    RR.check(d, got, want)
    return bits


def has(bits, *names):
    missing = [n for n in names if not bits >> jpeg.ROUTES[n] & 1]
    assert not missing, "routes %s not taken (taken: %s)" % (missing, jpeg.route_names(bits))


def lacks(bits, *names):
    there = [n for n in names if bits >> jpeg.ROUTES[n] & 1]
    assert not there, "routes %s taken (taken: %s)" % (there, jpeg.route_names(bits))


@pytest.fixture(autouse=True)
def _fresh_thread_buffers():
    jpeg.debug_configure("")
    jpeg.trim()
    yield
    jpeg.debug_configure("")


def test_fused_kernel_and_direct_stores_into_pinned_storage():
    bits = run(case(640, 480, "encode_device_into", dest="roomy", mem="pinned", content="photo"))
    has(bits, "FUSED", "FUSED_DIRECT")
    lacks(bits, "TWO_KERNEL")


def test_fused_segments_for_the_images_of_a_wide_batch():
    has(run(case(1024, 64, "batch_device", batch=4)), "FUSED_SEGMENTED", "BATCH_FUSED")


def test_restart_intervals_below_and_above_96_blocks():
    has(run(case(300, 200, "encode_device", ct=0, ss=0, restart=50)), "MULTI_PASS")  # gray: 50 blocks per segment
    bits = run(case(300, 200, "encode_device", ct=0, ss=0, restart=100, opt=True))
    has(bits, "SEGMENTED_TUPLE", "SINGLE_PASS_TUPLE")


def test_two_small_progressive_files_store_directly():
    run(case(200, 150, "encode", prog=True))
    has(run(case(200, 150, "encode", prog=True, cseed=6)), "PROG_SINGLE_PASS", "PROG_DIRECT_SMALL")


@pytest.mark.parametrize("mem", ["pageable"])
def test_noise_at_q100_after_a_small_file_grows_the_output_buffer(mem):
    run(case(16, 16, "encode_device_into", dest="roomy", mem=mem, content="flat"))
    has(run(case(700, 500, "encode_device_into", q=100, ss=0, dest="roomy", mem=mem)), "RESTUFF_GROW")


def test_noise_at_q100_into_device_memory_grows_the_output_buffer():
    run(case(16, 16, "batch_device", batch=2, content="flat"))
    has(run(case(700, 500, "batch_device", q=100, ss=0, batch=2)), "RESTUFF_GROW")


@pytest.mark.parametrize("entry,mem", [("encode_into_buffer", "pageable"), ("encode_into_buffer", "pinned"),
                                       ("encode_device_into", "pinned"), ("batch_device_into", "pinned")])
def test_short_caller_storage_is_refused_then_retried(entry, mem):
    kw = dict(batch=3) if entry.startswith("batch") else {}
    has(run(case(300, 200, entry, dest="short", mem=mem, **kw)), "CALLER_RETRY")


def test_size_queries_are_not_caller_retries():
    """The batch entries are asked for their sizes first (a null arena): that answer is no refused storage."""
    lacks(run(case(300, 200, "batch_device_into", batch=3, dest="roomy", mem="pinned")), "CALLER_RETRY")
    lacks(run(case(300, 200, "encode_device_into", dest="exact", mem="pinned")), "CALLER_RETRY")


def test_wide_and_narrow_batches():
    has(run(case(1024, 64, "batch_device", batch=4)), "BATCH_FUSED")
    has(run(case(640, 48, "batch_device", batch=4)), "BATCH_TWO_KERNEL")


def test_sub_batches():
    jpeg.debug_configure("batch_parts=3")
    has(run(case(320, 240, "batch_device_into", batch=6, dest="roomy", mem="pinned")), "SUB_BATCHES")


def test_sub_batches_never_hold_a_single_image():
    """Regression (python tests/route_runner.py 7014 11 1 batch_parts=3 batch1): batch_parts=3 on a batch of three cut it into
    sub-batches of one image, which took the single-image path and left no image starts to lay the files out by."""
    jpeg.debug_configure("batch_parts=3")
    run(case(56, 286, "batch_device_into", batch=3, q=100, ss=0, dest="roomy", mem="pinned"))
    has(run(case(186, 16, "batch_device_into", batch=5, q=100, ct=0, ss=0, dest="roomy", mem="pinned")), "SUB_BATCHES")


def test_pieces_that_start_over_write_the_headers_once():
    """Regression (python tests/route_runner.py 7015 3 1 bands_upload_min_mb=1,bands_upload_mb=1 host1mb): a scan in pieces
    that outgrows its guesses is coded again in one piece; that pass stored the file behind the headers written TWICE (the
    pieces attempt had appended them already) — 623 bytes too many, from the scan's first byte on."""
    jpeg.debug_configure("bands_upload_min_mb=1,bands_upload_mb=1")
    d = case(1064, 856, "encode", q=99, content="binary", cseed=553741997)
    has(run(d), "HOST_BANDS", "PIECES", "PIECES_REDO")


def test_large_dense_host_image_after_a_flat_one():
    """The same start-over without any switch: host pixels of 96 MiB and more are coded in pieces (unaligned width: the whole
    image first), dense content outgrows the pieces' guesses, and the flat file before it makes the file count as small (the
    stuffing kernel then stores into pinned memory behind the headers)."""
    run(case(64, 64, "encode", content="flat"))
    has(run(case(8200, 4096, "encode", q=100, content="binary", cseed=7)), "HOST_BANDS", "PIECES", "PIECES_REDO")


def test_load_forms_and_coefficient_forms():
    has(run(case(3, 9, "coefficients_device", offset=0)), "LOAD_BYTES", "COEF_SCALAR")
    has(run(case(100, 9, "coefficients_device", offset=1)), "LOAD_FUNNEL")
    has(run(case(100, 9, "coefficients_device", offset=0)), "LOAD_ALIGNED")
    jpeg.debug_configure("coef_form=packed")
    for w, h, ct, off in [(17, 15, 0, 3), (513, 9, 2, 1), (1537, 17, 0, 2), (2, 2, 2, 0)]:  # packed forms on edge tiles
        has(run(case(w, h, "coefficients_device", ct=ct, ss=0 if ct == 0 else 1, offset=off, q=97)), "COEF_PACKED")


def test_bands_over_devices():
    has(run(case(700, 300, "encode_multi", k=3)), "BANDS_MULTI")


# ---- grow pairs: a small call, then one that grows the buffer on a route that handed an earlier pointer to a kernel ----
# (buffer, first call, second call, a route the second call must take)
GROW_PAIRS = [
    ("d_px / d_coef / h_coef", case(64, 64, "encode", ct=0, ss=0, opt=True),
     case(1500, 1100, "encode", ct=0, ss=0, opt=True), "TWO_KERNEL"),
    ("h_file (fused, direct)", case(32, 32, "encode_device"), case(1800, 1200, "encode_device", q=100), "RESTUFF_GROW"),
    ("h_segs (segments, optimised tables)", case(64, 64, "encode_device", restart=4),
     case(1200, 900, "encode_device", restart=75, opt=True), "SEGMENTED_TUPLE"),
    ("e_out (segmented tuple)", case(64, 64, "encode_device", ct=0, ss=0, restart=12),
     case(1600, 1200, "encode_device", ct=0, ss=0, q=100, restart=200), "SEGMENTED_TUPLE"),
    ("e_pc_state / e_pc_spill (fused kernel, dense groups)", case(40, 40, "encode_device_into", dest="roomy", mem="pinned"),
     case(2100, 1100, "encode_device_into", q=100, ss=0, dest="roomy", mem="pinned"), "FUSED"),
    ("e_seg_* (multi-pass restart segments)", case(40, 40, "encode_device", ct=0, ss=0, restart=5),
     case(1500, 1000, "encode_device", ct=0, ss=0, restart=7, q=95), "MULTI_PASS"),
    ("e_stuff_state (progressive)", case(48, 48, "encode", prog=True), case(1500, 1100, "encode", prog=True, q=100),
     "PROG_SINGLE_PASS"),
]


@pytest.mark.parametrize("name,first,second,route", GROW_PAIRS, ids=[g[0] for g in GROW_PAIRS])
def test_grow_pair(name, first, second, route):
    run(first)
    has(run(second), route)
    run(first)  # and back: the grown buffers serve a small file again
