"""PNG batch entries on the device: `batch` equally sized images in one pass of filters, DEFLATE and CRC.  Throughout, file i
of a batch is held against the single-image entry's file for the same image, called separately in the same process: byte for
byte.  The single entry runs the same DEFLATE tail with a table of one segment, so that equality shows that segments do not
disturb each other (no match, offset, checksum or CRC piece crosses two images), not that the tail is right.  What pins the
bytes themselves is independent of both: the fixtures (tests/golden/png_files.json, made by the reference's own wasm build),
held against the files here where they exist, and tests/golden/png_own_bytes.json (tests/test_gpu_png_own_bytes.py), the
digests of every entry's output recorded while single and batch entries were separate code.

The fixture options carry NO_RAYON (the wasm build's semantics, which the stored streams were made with).  With it preset
0's AdaptiveFast is the sequential form, which prepares image by image: those groups set PNG_BATCH only.  The two preset-0
groups are therefore encoded a second time without NO_RAYON, where the filters run as one launch (PNG_BATCH_FILTER)."""
import collections
import hashlib
import struct
import zlib

import numpy as np
import pytest

import png_file_cases as PF
import synth

pytestmark = pytest.mark.gpu

STRATEGIES = list(range(9))


def png():
    from pixo_amd import png as P
    return P


def cuda(px):
    import torch
    return torch.from_numpy(np.ascontiguousarray(px, dtype=np.uint8).reshape(-1).copy()).cuda()


def routes(clear=True):
    from pixo_amd import _lib
    return int(_lib.load().pixo_hip_debug_routes(1 if clear else 0))


def opts(w, h, ct, preset=0, strategy=None, flags=0, quantization=None):
    from pixo_amd import ColorType
    P = png()
    b = P.PngOptions.builder(w, h).color_type(ColorType(ct)).preset(preset).flags(flags)
    if strategy is not None:
        b = b.filter_strategy(P.FilterStrategy(strategy))
    o = b.build()
    if quantization is not None:
        o.quantization = quantization
    return o


def singles(images, o):
    return [png().encode_device(cuda(px), o) for px in images]


def batch_of(images, o):
    return png().encode_batch_device(cuda(np.concatenate(images)), o, len(images))


def inflate(file_bytes):
    idat, other = PF.parse(file_bytes)  # (checks every chunk's CRC)
    return zlib.decompress(b"".join(idat)), idat, other


def noise_image(w, h, bpp, seed):
    return synth.lcg_bytes(w * h * bpp, seed)


def photo_like(w, h, bpp, seed):
    """scene content in any colour type: RGB as made, the others from its channels (images too small for it: noise)"""
    if min(w, h) < 16:
        return noise_image(w, h, bpp, seed)
    rgb = synth.scene(w, h, seed).reshape(h, w, 3)
    if bpp == 3:
        return rgb.reshape(-1)
    if bpp == 1:
        return rgb[:, :, 1].reshape(-1).copy()
    if bpp == 2:
        return np.stack([rgb[:, :, 1], 255 - rgb[:, :, 0] // 2], axis=2).reshape(-1)
    return np.concatenate([rgb, 255 - rgb[:, :, :1] // 3], axis=2).reshape(-1)


# ---- 1. fixture groups ---------------------------------------------------------------------------------------------------

GROUPS = collections.OrderedDict()
for _c in PF.CASES:
    GROUPS.setdefault((_c["w"], _c["h"], _c["color_type"], _c["preset"]), []).append(_c)
GROUPS = collections.OrderedDict((k, v) for k, v in GROUPS.items() if len(v) > 1)


def test_the_six_fixture_groups_are_there():
    assert sorted((k, len(v)) for k, v in GROUPS.items()) == sorted([
        ((128, 96, 2, 2), 3), ((97, 53, 2, 1), 3), ((512, 512, 2, 0), 2), ((512, 512, 2, 1), 3), ((512, 512, 3, 0), 3), ((512, 512, 3, 1), 2)])


@pytest.mark.parametrize("key", list(GROUPS), ids=["%dx%d_c%d_p%d" % k for k in GROUPS])
def test_fixture_group(key):
    P, cases = png(), GROUPS[key]
    images = [PF.make_input(c) for c in cases]
    o = PF.options(cases[0])
    want = singles(images, o)
    routes()
    got = batch_of(images, o)
    r = routes()
    assert r & P.ROUTE_PNG_BATCH and not r & P.ROUTE_PNG_BATCH_FILTER and not r & P.ROUTE_SUB_BATCHES  # NO_RAYON or reductions: image by image in
    for c, file_bytes, single in zip(cases, got, want):
        assert file_bytes == single, c["name"]
        stream, idat, other = inflate(file_bytes)
        assert [[t, b.hex()] for t, b in other] == c["chunks"], "a chunk around IDAT differs from the reference's"
        assert len(stream) == c["stream_len"] and hashlib.sha256(stream).hexdigest() == c["stream_sha256"]
        assert struct.unpack(">I", b"".join(idat)[-4:])[0] == c["adler32"] == zlib.adler32(stream)
    if key[3] == 0:  # ... and the parallel AdaptiveFast: the batched way in
        o.flags = 0
        want = singles(images, o)
        routes()
        got = batch_of(images, o)
        r = routes()
        assert r & P.ROUTE_PNG_BATCH and r & P.ROUTE_PNG_BATCH_FILTER
        for c, file_bytes, single in zip(cases, got, want):
            assert file_bytes == single, c["name"]
            stream, _, other = inflate(file_bytes)
            assert [[t, b.hex()] for t, b in other] == c["chunks"] and len(stream) == c["stream_len"]


# ---- 2. chunk edges ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,stream_len", [(254, 257, 65535), (255, 256, 65536)])
def test_chunk_edges(w, h, stream_len):
    images = [photo_like(w, h, 1, 20 + i) for i in range(3)]
    d_all = cuda(np.concatenate(images))
    d_one = [cuda(px) for px in images]
    for s in STRATEGIES:
        o = opts(w, h, 0, strategy=s)
        got = png().encode_batch_device(d_all, o, 3)
        for i in range(3):
            assert got[i] == png().encode_device(d_one[i], o), (s, i)
        assert len(inflate(got[0])[0]) == stream_len


# ---- 3. no match across images ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,stream_len", [(64, 64, 12352), (200, 150, 90150)])
@pytest.mark.parametrize("effort", [0, 1])
def test_no_match_across_images(w, h, stream_len, effort):
    px = photo_like(w, h, 3, 31)
    o = opts(w, h, 2, flags=png().EFFORT_HIGH if effort else 0)
    single = png().encode_device(cuda(px), o)
    got = batch_of([px] * 4, o)
    assert got == [single] * 4
    for file_bytes in got:
        assert len(inflate(file_bytes)[0]) == stream_len


# ---- 4. IDAT boundary ----------------------------------------------------------------------------------------------------

def test_idat_boundary():
    w, h = 300, 220
    images = [noise_image(w, h, 4, 40 + i) for i in range(3)]
    o = opts(w, h, 3)
    want = singles(images, o)
    for file_bytes in want:
        stream, idat, _ = inflate(file_bytes)
        assert len(stream) == 264220 and len(idat) == 2 and len(idat[0]) == 262144
    assert batch_of(images, o) == want


# ---- 5. tiny and odd -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,ct,n", [(37, 29, 2, 1), (1, 1, 2, 3), (5, 3, 1, 2), (61, 47, 0, 3), (61, 47, 1, 3), (61, 47, 2, 3), (61, 47, 3, 3)])
def test_tiny_and_odd(w, h, ct, n):
    images = [photo_like(w, h, ct + 1, 50 + i) for i in range(n)]
    for preset in (0, 1):
        o = opts(w, h, ct, preset=preset)
        assert batch_of(images, o) == singles(images, o), preset


# ---- 6. sequential AdaptiveFast ------------------------------------------------------------------------------------------

def _first_row_winner_images(w, h):
    """Three images whose first rows are won by different filters.  Row 0 has no row above, so Up leaves its bytes as they are
    and Paeth equals Sub there.  Constant rows: Sub's residuals vanish behind the first pixel, Up pays for every byte.  Pixels that
    alternate between 3 and 253 (-3 as i8): Up scores 3 a byte, Sub 6.  A ramp: Sub scores 3 a byte, Up the bytes themselves."""
    x, y = np.arange(w)[None, :, None], np.arange(h)[:, None, None]
    a = np.broadcast_to((y * 40 + 100) & 255, (h, w, 3)).astype(np.uint8)
    b = np.broadcast_to(np.where((x + y) % 2 == 0, 3, 253), (h, w, 3)).astype(np.uint8)
    c = np.broadcast_to((x * 3 + y * 7) & 255, (h, w, 3)).astype(np.uint8)
    return [a.reshape(-1).copy(), b.reshape(-1).copy(), c.reshape(-1).copy()]


# (96 x 20 is 1,920 pixels: areas up to 4,096 take the Sub rule, so its rows cannot differ — it is kept as a batch that must
# equal its single files; 300 x 20 is the height <= 32 case in which the sequential AdaptiveFast really runs)
@pytest.mark.parametrize("w,h,flags", [(96, 20, 0), (300, 20, 0), (128, 96, 1)])
def test_sequential_adaptive_fast(w, h, flags):
    P = png()
    images = _first_row_winner_images(w, h)
    o = opts(w, h, 2, strategy=int(P.FilterStrategy.ADAPTIVE_FAST), flags=flags)
    want = singles(images, o)
    row1 = [inflate(f)[0][3 * w + 1] for f in want]
    print("filter bytes of row 1:", row1)
    assert len(set(row1)) > 1 or w * h <= 4096, "the images' first-row winners are all the same"
    routes()
    assert batch_of(images, o) == want
    r = routes()
    # (under the Sub rule nothing is decided by row 0: those images take the batched way in)
    assert r & P.ROUTE_PNG_BATCH and bool(r & P.ROUTE_PNG_BATCH_FILTER) == (w * h <= 4096)


# ---- 7. lossy -------------------------------------------------------------------------------------------------------------

def test_lossy():
    P = png()
    w, h = 128, 96
    images = [photo_like(w, h, 4, 70 + i) for i in range(3)]
    q = P.QuantizationOptions(P.QuantizationMode.FORCE, 64, True)
    for preset in (0, 1):
        o = opts(w, h, 3, preset=preset, quantization=q)
        want = singles(images, o)
        assert all(f[25] == 3 for f in want), "the forced files are not indexed"
        assert batch_of(images, o) == want
    # Auto declines on an image of few colours (not more than max_colors): its file is the lossless one
    few = np.tile(np.array([[10, 20, 30, 255], [200, 100, 50, 255]], np.uint8), (w * h // 2, 1)).reshape(-1)
    o = opts(w, h, 3, preset=1, quantization=P.QuantizationOptions(P.QuantizationMode.AUTO, 256, True))
    mixed = [images[0], few, images[1]]
    want = singles(mixed, o)
    assert want[1] == P.encode_device(cuda(few), opts(w, h, 3, preset=1)), "the gate did not decline"
    assert batch_of(mixed, o) == want


# ---- 8. sub-batch boundary -----------------------------------------------------------------------------------------------

def test_sub_batch_boundary():
    from pixo_amd import _lib
    P, L = png(), _lib.load()
    w, h = 128, 96
    images = [photo_like(w, h, 3, 80 + i) for i in range(7)]
    o = opts(w, h, 2)
    want = singles(images, o)
    stream = h * (3 * w + 1)
    L.pixo_hip_debug_configure(("png_batch_bytes=%d" % (stream * 5 // 2)).encode())
    try:
        routes()
        got = batch_of(images, o)
        r = routes()
    finally:
        L.pixo_hip_debug_configure(None)
    assert r & P.ROUTE_SUB_BATCHES and r & P.ROUTE_PNG_BATCH_FILTER
    assert got == want
    routes()
    assert batch_of(images, o) == want and not routes() & P.ROUTE_SUB_BATCHES


def test_sub_batches_are_capped_by_chunks():
    """The DEFLATE scratch is per chunk (about 328 KB each, however short the chunk) and every image has at least one: a
    sub-batch holds at most 1024 chunks.  1100 images of 8 x 8 are 215 KB of stream — far below the byte limit — and two
    sub-batches; 1024 of them are one."""
    P = png()
    w = h = 8
    one = w * h * 3
    pixels = noise_image(w, h * 1100, 3, 300).copy()
    pixels.reshape(1100, one)[::2] = (np.arange(550, dtype=np.uint8) * 3)[:, None]  # every other image is flat, each another value
    o = opts(w, h, 2)
    d_all = cuda(pixels)
    routes()
    got = P.encode_batch_device(d_all, o, 1100)
    assert routes() & P.ROUTE_SUB_BATCHES
    for i in list(range(0, 1100, 41)) + [1022, 1023, 1024, 1025, 1099]:  # a sample, and both sides of the boundary
        assert got[i] == P.encode_device(d_all[i * one:(i + 1) * one], o), i
    assert len(set(got)) > 600
    routes()
    assert P.encode_batch_device(d_all[:1024 * w * h * 3], o, 1024) == got[:1024] and not routes() & P.ROUTE_SUB_BATCHES
    # two chunks an image: 512 images are one sub-batch, 513 are two
    w, h = 200, 150
    d_two = cuda(np.concatenate([photo_like(w, h, 3, 31)] * 513))
    o = opts(w, h, 2)
    routes()
    got = P.encode_batch_device(d_two, o, 513)
    assert routes() & P.ROUTE_SUB_BATCHES and got == [got[0]] * 513 and got[0] == P.encode_device(d_two[:w * h * 3], o)
    routes()
    assert P.encode_batch_device(d_two[:512 * w * h * 3], o, 512) == got[:512] and not routes() & P.ROUTE_SUB_BATCHES


def test_device_arena_is_refused():
    import torch
    from pixo_amd.error import Error as PixoError
    o = opts(8, 8, 2)
    d_all = cuda(np.zeros(8 * 8 * 3 * 2, np.uint8))
    with pytest.raises(PixoError):
        png().encode_batch_device_into(torch.zeros(4096, dtype=torch.uint8, device="cuda"), d_all, o, 2)
    assert len(png().encode_batch_device(d_all, o, 2)) == 2


# ---- 9. into an arena ----------------------------------------------------------------------------------------------------

def test_into_arena():
    import torch
    from pixo_amd.error import BufferTooSmall
    P = png()
    w, h = 61, 47
    images = [photo_like(w, h, 3, 90 + i) for i in range(3)]
    o = opts(w, h, 2)
    d_all = cuda(np.concatenate(images))
    want = P.encode_batch_device(d_all, o, 3)
    offsets, lens = P.encode_batch_device_into(None, d_all, o, 3)  # the size query
    assert lens == [len(f) for f in want] and offsets == [0, lens[0], lens[0] + lens[1]]
    total = offsets[-1] + lens[-1]
    # pageable and pinned, each at an even and at an odd address: every file then lies at an odd one in one of the two
    for base in (torch.full((total + 8,), 0xEE, dtype=torch.uint8), torch.full((total + 8,), 0xEE, dtype=torch.uint8).pin_memory(),
                 np.full(total + 8, 0xEE, np.uint8)):
        for shift in (0, 1):
            arena = base[shift:]
            assert P.encode_batch_device_into(arena, d_all, o, 3) == (offsets, lens)
            flat = arena.numpy() if hasattr(arena, "numpy") else arena
            assert [flat[a:a + n].tobytes() for a, n in zip(offsets, lens)] == want
            assert bytes(flat[total:]) == b"\xEE" * (flat.size - total)
    short = np.full(total - 1, 0xEE, np.uint8)
    with pytest.raises(BufferTooSmall) as e:
        P.encode_batch_device_into(short, d_all, o, 3)
    assert str(e.value) == "output buffer too small: need %d bytes" % total
    assert (e.value.offsets, e.value.lens, e.value.needed) == (offsets, lens, total)
    assert bytes(short) == b"\xEE" * (total - 1), "the refused call wrote into the arena"
    assert P.encode_batch_device(d_all, o, 3) == want  # the next call on the same thread


# ---- 10. host entry ------------------------------------------------------------------------------------------------------

def test_host_entry():
    P = png()
    w, h = 97, 53
    images = [photo_like(w, h, 4, 100 + i) for i in range(3)]
    for preset in (0, 1):
        o = opts(w, h, 3, preset=preset)
        got = P.encode_batch(np.concatenate(images), o, 3)
        assert got == batch_of(images, o) == singles(images, o)
        assert P.encode_batch(np.concatenate(images), o, 3) == got


# ---- 11. state -----------------------------------------------------------------------------------------------------------

def test_state_between_larger_and_smaller_single_calls():
    P = png()
    big, mid, small = photo_like(400, 300, 3, 110), [photo_like(128, 96, 3, 111 + i) for i in range(3)], photo_like(33, 21, 3, 115)
    o_big, o_mid, o_small = opts(400, 300, 2, preset=1), opts(128, 96, 2), opts(33, 21, 2)
    want = (P.encode_device(cuda(big), o_big), singles(mid, o_mid), P.encode_device(cuda(small), o_small))
    for _ in range(2):
        got = (P.encode_device(cuda(big), o_big), batch_of(mid, o_mid), P.encode_device(cuda(small), o_small))
        assert got == want


def test_device_wrappers_check_the_tensor():
    o = opts(8, 8, 2)
    with pytest.raises(ValueError):
        png().encode_batch_device(cuda(np.zeros(8 * 8 * 3 * 2, np.uint8)), o, 3)
