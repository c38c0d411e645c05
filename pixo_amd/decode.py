"""`pixo::decode` on the MI355X (reference src/decode/png.rs, src/decode/jpeg.rs): a PNG or baseline JPEG file -> 8-bit pixels.  The chunk walk, its checks and the
inflate run on the host, in the reference's order and with its messages; row reconstruction and the conversion to pixels run
on the device — and, for the batch entries with `device_inflate=True`, the inflate too (one wavefront per stream; the single entries
keep the host inflate: one stream is one wavefront).  Mirrors `PngImage` and `decode_png`; `decode_png_info` and `decode_png_device` are what a caller needs to keep
the pixels in device memory for `resize.resize_device`, `jpeg.encode_device` and `png.encode_device`.  JPEG decode (`decode_jpeg*`, below): marker walk and
Huffman decode on the host, IDCT, upsampling and colour conversion on the device, pinned byte for byte to libjpeg-turbo's
defaults, not to the reference's decoder.  No CPU fallback."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._images import flat_u8, image_bytes
from .color import ColorType


@dataclass(frozen=True)
class PngImage:
    """png.rs:18-28"""
    width: int
    height: int
    pixels: bytes
    color_type: ColorType


def _file(data) -> np.ndarray:
    return flat_u8(data if isinstance(data, np.ndarray) else bytes(data))


def pass_rows() -> int:
    """Rows a workgroup of the reconstruction kernel walks side by side (png_unfilter.hpp kUnfilterPassRows)."""
    return int(_lib.load().pixo_hip_png_unfilter_pass_rows())


def decode_png(data) -> PngImage:
    """A PNG file (bytes) -> PngImage with host pixels."""
    L = _lib.load()
    f = _file(data)
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    w, h, ct = C.c_uint32(), C.c_uint32(), C.c_uint8()
    rc = L.pixo_hip_png_decode(f.ctypes.data, f.size, C.byref(out), C.byref(n), C.byref(w), C.byref(h), C.byref(ct))
    _lib.check(rc)
    return PngImage(w.value, h.value, _lib.take(L, out, n), ColorType(ct.value))


def decode_png_info(data):
    """(width, height, ColorType) of the pixels decode_png would return: the walk and its checks only — no inflate, no GPU."""
    L = _lib.load()
    f = _file(data)
    w, h, ct = C.c_uint32(), C.c_uint32(), C.c_uint8()
    _lib.check(L.pixo_hip_png_decode_info(f.ctypes.data, f.size, C.byref(w), C.byref(h), C.byref(ct)))
    return w.value, h.value, ColorType(ct.value)


def decode_png_device(data, out=None, stream=None):
    """A PNG file (host bytes) -> a uint8 torch tensor (height, width, channels) on the current device.  Enqueue only: the
    upload and the kernels run on `stream` (a raw stream handle; default the current torch stream) behind the work of the
    producer stream.  `out`: a contiguous uint8 device tensor to decode into; BufferTooSmall carries the bytes needed in
    `.needed`.  Returns (tensor, ColorType)."""
    import torch
    L = _lib.load()
    f = _file(data)
    w, h, ct = C.c_uint32(), C.c_uint32(), C.c_uint8()
    if out is None:
        iw, ih, ict = decode_png_info(f)
        out = torch.empty((ih, iw, ict.bytes_per_pixel()), dtype=torch.uint8, device="cuda")
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.is_cuda
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    rc = L.pixo_hip_png_decode_device(f.ctypes.data, f.size, out.data_ptr(), _lib.nbytes(out), C.byref(w), C.byref(h), C.byref(ct),
                                      C.c_void_p(stream) if stream else None)
    _lib.check(rc, needed=w.value * h.value * ColorType(ct.value).bytes_per_pixel() if rc == -9 else None)
    color = ColorType(ct.value)
    n = w.value * h.value * color.bytes_per_pixel()
    return out.reshape(-1)[:n].view(h.value, w.value, color.bytes_per_pixel()), color


# ---- batches: N files -> N images back to back in device memory, one launch per pass (include/pixo_hip.h) ----------------------
ROUTES = {"PNG_DECODE_BATCH": 42}  # the route record's bit of the batch entries (csrc/routes.hpp; read with jpeg.routes)
ROUTE_PNG_DECODE_BATCH = 1 << ROUTES["PNG_DECODE_BATCH"]
ONE_THREAD = 1  # PIXO_DECODE_ONE_THREAD
DEVICE_INFLATE = 2  # PIXO_DECODE_DEVICE_INFLATE: the batch entries inflate on the device (opt-in)
# ... and the bits of that path (a dict of its own: ROUTES above is the complete list of the batch entries' own bit)
INFLATE_ROUTES = {"PNG_INFLATE_DEVICE": 43, "PNG_INFLATE_HOST_REDO": 44}
INFLATE_OK, INFLATE_FAILED, INFLATE_NEEDS_HOST = 0, 1, 2  # the device verdicts (png_inflate_math.h)


DEVICE_ENTROPY = 4  # PIXO_DECODE_DEVICE_ENTROPY: the JPEG batch entries decode the Huffman scans on the device (opt-in)
# ... and the bits of that path
ENTROPY_ROUTES = {"JPEG_ENTROPY_DEVICE": 50, "JPEG_ENTROPY_HOST_REDO": 51}
ROUTE_JPEG_ENTROPY_DEVICE = 1 << ENTROPY_ROUTES["JPEG_ENTROPY_DEVICE"]
ROUTE_JPEG_ENTROPY_HOST_REDO = 1 << ENTROPY_ROUTES["JPEG_ENTROPY_HOST_REDO"]
# why the device does not vouch for a file (jpeg_entropy_dec_math.h; 4: the host decodes the file from the start)
ENTROPY_VOUCHED, ENTROPY_CHAIN_DEAD, ENTROPY_NOT_SETTLED, ENTROPY_SHORT, ENTROPY_HOST = 0, 1, 2, 3, 4


def _flags(one_thread, device_inflate, device_entropy=False) -> int:
    return (ONE_THREAD if one_thread else 0) | (DEVICE_INFLATE if device_inflate else 0) | (DEVICE_ENTROPY if device_entropy else 0)


def _files_c(files):
    """The files as the C array, and the arrays that keep their bytes alive"""
    held = [_file(f) for f in files]
    arr = (_lib.PngFileC * max(len(held), 1))()
    for i, f in enumerate(held):
        arr[i] = _lib.PngFileC(f.ctypes.data, f.size)
    return arr, held


def decode_png_batch_info(files):
    """([(width, height, ColorType, offset)], total) of the block decode_png_batch_device writes: image i at `offset`, every
    offset a multiple of 16, `total` the end of the last image.  The walks and their checks only — no inflate, no GPU."""
    L = _lib.load()
    arr, held = _files_c(files)
    images, total = (_lib.PngImageC * max(len(held), 1))(), C.c_size_t()
    _lib.check(L.pixo_hip_png_decode_batch_info(arr, len(held), images, C.byref(total)))
    return [(im.width, im.height, ColorType(im.color_type), im.offset) for im in images[:len(held)]], total.value


def decode_png_batch(files, one_thread=False, device_inflate=False) -> list:
    """PNG files (bytes) -> [PngImage] with host pixels, image i what decode_png makes of file i.  The inflates run on up to 8
    host threads unless `one_thread` — or, with `device_inflate`, on the device, all streams of a sub-batch in one launch; the host
    then inflates again only the streams the device did not vouch for (on those threads).  The images are the same bytes."""
    L = _lib.load()
    arr, held = _files_c(files)
    images = (_lib.PngImageC * max(len(held), 1))()
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    _lib.check(L.pixo_hip_png_decode_batch(arr, len(held), _flags(one_thread, device_inflate), C.byref(out), C.byref(n), images))
    block = _lib.take(L, out, n)
    return [PngImage(im.width, im.height, block[im.offset:im.offset + image_bytes(im)], ColorType(im.color_type)) for im in images[:len(held)]]


def decode_png_batch_device(files, out=None, stream=None, one_thread=False, device_inflate=False) -> list:
    """PNG files (host bytes) -> [(uint8 tensor view (height, width, channels), ColorType)], views into ONE uint8 device
    tensor: `out` (contiguous, any alignment; the bytes between two images are left as they are), or one allocated from
    decode_png_batch_info.  Enqueue only, ordered like decode_png_device; BufferTooSmall carries the total in `.needed`.  The
    views are what resize.resize_batch_device takes as sources (grouped by colour type).  `device_inflate`: as decode_png_batch;
    the call then waits on the host once per sub-batch, and after a refusal that only the inflated streams show `out` is unspecified."""
    import torch
    L = _lib.load()
    arr, held = _files_c(files)
    images = (_lib.PngImageC * max(len(held), 1))()
    if out is None:
        out = torch.empty(max(decode_png_batch_info(held)[1], 1), dtype=torch.uint8, device="cuda")
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.is_cuda
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    rc = L.pixo_hip_png_decode_batch_device(arr, len(held), _flags(one_thread, device_inflate), out.data_ptr(), _lib.nbytes(out), images,
                                            C.c_void_p(stream) if stream else None)
    last = images[len(held) - 1] if held else None
    _lib.check(rc, needed=last.offset + image_bytes(last) if rc == -9 else None)
    flat = out.reshape(-1)
    return [(flat[im.offset:im.offset + image_bytes(im)].view(im.height, im.width, ColorType(im.color_type).bytes_per_pixel()), ColorType(im.color_type))
            for im in images[:len(held)]]


def decode_png_batch_plan(files, one_thread=False) -> dict:
    """What the batch entries decide for these files, computed on the host (no GPU): `sub_first` (where each sub-batch starts,
    and the batch's end), `runs` (workgroups that reconstruct each image), `unfilter_launches` and `convert_launches` (summed
    over the sub-batches) and `threads` (host threads that inflated).  Refuses as the decode entries do."""
    L = _lib.load()
    arr, held = _files_c(files)
    n = len(held)
    sub_first, runs = (C.c_uint32 * (n + 1))(), (C.c_uint64 * max(n, 1))()
    subs, unfilter, convert, threads = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    _lib.check(L.pixo_hip_debug_png_decode_batch_plan(arr, n, ONE_THREAD if one_thread else 0, sub_first, C.byref(subs), runs, C.byref(unfilter),
                                                      C.byref(convert), C.byref(threads)))
    return dict(sub_first=list(sub_first[:subs.value + 1]), runs=list(runs[:n]), unfilter_launches=unfilter.value,
                convert_launches=convert.value, threads=threads.value)


def inflate_zlib(data, expected: int) -> bytes:
    """The host inflate alone (inflate.rs:294-352 with Some(expected)); no GPU."""
    L = _lib.load()
    f = _file(data)
    out = np.empty(max(expected, 1), np.uint8)
    _lib.check(L.pixo_hip_zlib_inflate(f.ctypes.data if f.size else out.ctypes.data, f.size, out.ctypes.data, expected))
    return out[:expected].tobytes()


def inflate_step_tokens() -> int:
    """Tokens a step of the device inflate holds at most (png_inflate_math.h kStepTokens)."""
    return int(_lib.load().pixo_hip_png_inflate_step_tokens())


def inflate_window_bytes() -> int:
    """Bytes of the device inflate's LDS ring (kWindowBytes)."""
    return int(_lib.load().pixo_hip_png_inflate_window_bytes())


def inflate_far_distance() -> int:
    """A match further back than this closes its step (kFarDistance)."""
    return int(_lib.load().pixo_hip_png_inflate_far_distance())


def inflate_stored_chunk() -> int:
    """Bytes of a stored block the device inflate copies at a time (kStoredChunk)."""
    return int(_lib.load().pixo_hip_png_inflate_stored_chunk())


def inflate_zlib_batch_debug(streams, expected, out, out_at):
    """The inflate kernel alone (pixo_hip_debug_zlib_inflate_batch_device): zlib streams (bytes, of any origin) inflated on the
    device into `out` — a uint8 numpy array the caller has filled, at least max(out_at[i] + expected[i]) bytes, uploaded whole and
    downloaded again — stream i into [out_at[i], out_at[i] + expected[i]).  No host inflate behind it.  Returns
    (verdicts, produced, adlers, kernel_ms)."""
    L = _lib.load()
    arr, held = _files_c(streams)
    n = len(held)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= max([a + e for a, e in zip(out_at, expected)] + [0])
    exp, at = (C.c_uint64 * max(n, 1))(*expected), (C.c_uint64 * max(n, 1))(*out_at)
    verdict, produced, adler, ms = (C.c_uint32 * max(n, 1))(), (C.c_uint64 * max(n, 1))(), (C.c_uint32 * max(n, 1))(), C.c_double()
    _lib.check(L.pixo_hip_debug_zlib_inflate_batch_device(arr, n, exp, out.ctypes.data, at, verdict, produced, adler, C.byref(ms)))
    return list(verdict[:n]), list(produced[:n]), list(adler[:n]), ms.value


# ---- JPEG decode: baseline files -> pixels, byte for byte libjpeg-turbo's defaults (include/pixo_hip.h) -------------------------
@dataclass(frozen=True)
class JpegImage:
    """jpeg.rs:22-31"""
    width: int
    height: int
    pixels: bytes
    color_type: ColorType


JPEG_CLASSES = ("gray", "444", "422", "420")  # pixo_hip_debug_jpeg_decode_batch_plan's classes


def decode_jpeg_tile_mcus():
    """(MCUs across, MCUs down) of the tile a workgroup of the decode kernel owns (jpeg_decode_math.h)."""
    x, y = C.c_uint32(), C.c_uint32()
    _lib.load().pixo_hip_jpeg_decode_tile_mcus(C.byref(x), C.byref(y))
    return x.value, y.value


def decode_jpeg(data) -> JpegImage:
    """A baseline JPEG file (bytes) -> JpegImage with host pixels: Gray for one component, Rgb for three."""
    L = _lib.load()
    f = _file(data)
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    w, h, ct = C.c_uint32(), C.c_uint32(), C.c_uint8()
    _lib.check(L.pixo_hip_jpeg_decode(f.ctypes.data, f.size, C.byref(out), C.byref(n), C.byref(w), C.byref(h), C.byref(ct)))
    return JpegImage(w.value, h.value, _lib.take(L, out, n), ColorType(ct.value))


def decode_jpeg_info(data):
    """(width, height, ColorType) of the pixels decode_jpeg would return: the walk up to SOS only — no entropy decode, no GPU."""
    L = _lib.load()
    f = _file(data)
    w, h, ct = C.c_uint32(), C.c_uint32(), C.c_uint8()
    _lib.check(L.pixo_hip_jpeg_decode_info(f.ctypes.data, f.size, C.byref(w), C.byref(h), C.byref(ct)))
    return w.value, h.value, ColorType(ct.value)


def decode_jpeg_device(data, out=None, stream=None):
    """A baseline JPEG file (host bytes) -> a uint8 torch tensor (height, width, channels) on the current device.  Enqueue
    only, ordered like decode_png_device.  `out`: a contiguous uint8 device tensor to decode into; BufferTooSmall carries the
    bytes needed in `.needed`.  Returns (tensor, ColorType)."""
    import torch
    L = _lib.load()
    f = _file(data)
    w, h, ct = C.c_uint32(), C.c_uint32(), C.c_uint8()
    if out is None:
        iw, ih, ict = decode_jpeg_info(f)
        out = torch.empty((ih, iw, ict.bytes_per_pixel()), dtype=torch.uint8, device="cuda")
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.is_cuda
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    rc = L.pixo_hip_jpeg_decode_device(f.ctypes.data, f.size, out.data_ptr(), _lib.nbytes(out), C.byref(w), C.byref(h), C.byref(ct),
                                       C.c_void_p(stream) if stream else None)
    _lib.check(rc, needed=w.value * h.value * ColorType(ct.value).bytes_per_pixel() if rc == -9 else None)
    color = ColorType(ct.value)
    n = w.value * h.value * color.bytes_per_pixel()
    return out.reshape(-1)[:n].view(h.value, w.value, color.bytes_per_pixel()), color


def decode_jpeg_batch_info(files):
    """([(width, height, ColorType, offset)], total) of the block decode_jpeg_batch_device writes, as decode_png_batch_info."""
    L = _lib.load()
    arr, held = _files_c(files)
    images, total = (_lib.PngImageC * max(len(held), 1))(), C.c_size_t()
    _lib.check(L.pixo_hip_jpeg_decode_batch_info(arr, len(held), images, C.byref(total)))
    return [(im.width, im.height, ColorType(im.color_type), im.offset) for im in images[:len(held)]], total.value


def decode_jpeg_batch(files, one_thread=False, device_entropy=False) -> list:
    """JPEG files (bytes) -> [JpegImage] with host pixels, image i what decode_jpeg makes of file i.  The scans are decoded on
    up to 8 host threads unless `one_thread` — or, with `device_entropy`, on the device (jpeg_entropy_dec.hip); the host then
    decodes again only the files the device did not vouch for.  The images, and a refusal's status and words, are the same."""
    L = _lib.load()
    arr, held = _files_c(files)
    images = (_lib.PngImageC * max(len(held), 1))()
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    _lib.check(L.pixo_hip_jpeg_decode_batch(arr, len(held), _flags(one_thread, False, device_entropy), C.byref(out), C.byref(n), images))
    block = _lib.take(L, out, n)
    return [JpegImage(im.width, im.height, block[im.offset:im.offset + image_bytes(im)], ColorType(im.color_type)) for im in images[:len(held)]]


def decode_jpeg_batch_device(files, out=None, stream=None, one_thread=False, records=False, device_entropy=False):
    """JPEG files (host bytes) -> [(uint8 tensor view (height, width, channels), ColorType)], views into ONE uint8 device
    tensor: `out` (contiguous, any alignment; the bytes between two images are left as they are), or one allocated from
    decode_jpeg_batch_info.  Enqueue only; BufferTooSmall carries the total in `.needed`.  `records`: also return the block and
    the pixo_png_image records, which resize.fit_images, resize.resize_images_device, convert, jpeg.encode_images_device and
    png.encode_images_device take unchanged: (views, out, images).  `device_entropy`: as decode_jpeg_batch; the call then waits
    on the host several times per sub-batch, and after a refusal that only the scans show `out` is unspecified."""
    import torch
    L = _lib.load()
    arr, held = _files_c(files)
    images = (_lib.PngImageC * max(len(held), 1))()
    if out is None:
        out = torch.empty(max(decode_jpeg_batch_info(held)[1], 1), dtype=torch.uint8, device="cuda")
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.is_cuda
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    rc = L.pixo_hip_jpeg_decode_batch_device(arr, len(held), _flags(one_thread, False, device_entropy), out.data_ptr(), _lib.nbytes(out), images,
                                             C.c_void_p(stream) if stream else None)
    last = images[len(held) - 1] if held else None
    _lib.check(rc, needed=last.offset + image_bytes(last) if rc == -9 else None)
    flat = out.reshape(-1)
    views = [(flat[im.offset:im.offset + image_bytes(im)].view(im.height, im.width, ColorType(im.color_type).bytes_per_pixel()), ColorType(im.color_type))
             for im in images[:len(held)]]
    return (views, out, images) if records else views


def decode_jpeg_batch_plan(files, one_thread=False, device_entropy=False) -> dict:
    """What the batch entries decide for these files, computed on the host (no GPU): `sub_first`, `classes` (per image, of
    JPEG_CLASSES), `launches` (summed over the sub-batches), `threads` and `on_device` (per image: with `device_entropy`, whether
    its scan goes to the device)."""
    L = _lib.load()
    arr, held = _files_c(files)
    n = len(held)
    sub_first, classes = (C.c_uint32 * (n + 1))(), (C.c_uint8 * max(n, 1))()
    subs, launches, threads = C.c_uint32(), C.c_uint32(), C.c_uint32()
    flags = _flags(one_thread, False, device_entropy)
    _lib.check(L.pixo_hip_debug_jpeg_decode_batch_plan(arr, n, flags, sub_first, C.byref(subs), classes, C.byref(launches), C.byref(threads)))
    on_device, sub_first2, subs2 = (C.c_uint8 * max(n, 1))(), (C.c_uint32 * (n + 1))(), C.c_uint32()
    _lib.check(L.pixo_hip_debug_jpeg_entropy_plan(arr, n, flags, on_device, sub_first2, C.byref(subs2)))
    return dict(sub_first=list(sub_first[:subs.value + 1]), classes=[JPEG_CLASSES[k] for k in classes[:n]], launches=launches.value,
                threads=threads.value, on_device=[bool(x) for x in on_device[:n]])


def decode_jpeg_batch_tables(files) -> np.ndarray:
    """The quantisation tables in the records the batch entries would hand the kernel: uint16 (images, 3, 64), natural order;
    zeros for the components a gray image lacks.  Host only (tests)."""
    L = _lib.load()
    arr, held = _files_c(files)
    out = np.zeros((len(held), 3, 64), np.uint16)
    _lib.check(L.pixo_hip_debug_jpeg_decode_batch_tables(arr, len(held), out.ctypes.data))
    return out


def decode_jpeg_coefficients(data, component: int) -> np.ndarray:
    """The quantised coefficients of one component as the host's entropy decoder read them: int16 (blocks down, blocks across,
    64), zigzag order within a block, the component's padded plane.  Host only (tests)."""
    L = _lib.load()
    f = _file(data)
    bw, bh = C.c_uint32(), C.c_uint32()
    rc = L.pixo_hip_debug_jpeg_decode_coefficients(f.ctypes.data, f.size, component, None, 0, C.byref(bw), C.byref(bh))
    if rc != -9:
        _lib.check(rc)
    out = np.zeros((bh.value, bw.value, 64), np.int16)
    if out.size:
        _lib.check(L.pixo_hip_debug_jpeg_decode_coefficients(f.ctypes.data, f.size, component, out.ctypes.data, out.size, C.byref(bw), C.byref(bh)))
    return out


def decode_jpeg_batch_timed(files, one_thread=False, device_entropy=False):
    """MEASUREMENT: decode_jpeg_batch with its legs timed -> [entropy decode, uploads, kernels, copy down, whole call] in ms.
    With `device_entropy` [0] is the host's share and decode_jpeg_entropy_last() gives the device leg."""
    L = _lib.load()
    arr, held = _files_c(files)
    ms = (C.c_double * 5)()
    _lib.check(L.pixo_hip_debug_jpeg_decode_batch_timed(arr, len(held), _flags(one_thread, False, device_entropy), ms))
    return list(ms)


def decode_jpeg_entropy_geometry() -> dict:
    """The device Huffman decode's geometry (jpeg_entropy_dec_math.h): `sub_bytes` of a subsequence, `group_subs` subsequences a
    workgroup owns, `round_cap` of a call, `min_scan_bytes` of a scan that goes to the device."""
    g = [C.c_uint32() for _ in range(4)]
    _lib.load().pixo_hip_jpeg_entropy_geometry(*[C.byref(x) for x in g])
    return dict(sub_bytes=g[0].value, group_subs=g[1].value, round_cap=g[2].value, min_scan_bytes=g[3].value)


def decode_jpeg_entropy_debug(files, component=0, round_cap=0):
    """The device Huffman decode alone (pixo_hip_debug_jpeg_entropy_batch; tests): per file a dict of `vouched`, `why` (ENTROPY_*),
    `subs`, `rounds` and `coef` — the coefficients of `component` as decode_jpeg_coefficients returns them, or None where the
    device does not vouch or the file has no such component.  No host decoder behind it."""
    L = _lib.load()
    arr, held = _files_c(files)
    n = len(held)
    shapes, at, total = [], [], 0
    for f in held:
        bw, bh = C.c_uint32(), C.c_uint32()
        rc = L.pixo_hip_debug_jpeg_decode_coefficients(f.ctypes.data, f.size, component, None, 0, C.byref(bw), C.byref(bh))
        if rc not in (0, -9):
            bw.value = bh.value = 0  # (no such component)
        shapes.append((bh.value, bw.value))
        at.append(total)
        total += bh.value * bw.value * 64
    out = np.zeros(max(total, 1), np.int16)
    info = (C.c_uint32 * (4 * max(n, 1)))()
    _lib.check(L.pixo_hip_debug_jpeg_entropy_batch(arr, n, component, round_cap, out.ctypes.data, (C.c_uint64 * max(n, 1))(*at), info))
    res = []
    for i in range(n):
        vouched = bool(info[4 * i])
        bh, bw = shapes[i]
        coef = out[at[i]:at[i] + bh * bw * 64].reshape(bh, bw, 64).copy() if vouched and bh * bw else None
        res.append(dict(vouched=vouched, why=info[4 * i + 1], subs=info[4 * i + 2], rounds=info[4 * i + 3], coef=coef))
    return res


def decode_jpeg_entropy_last() -> dict:
    """MEASUREMENT: of this thread's last batch call with `device_entropy` — `device_ms` (the entropy launches and the waits
    between them), `rounds` (the most a file used), `files_device`, `files_redone`."""
    ms, r, d, h = C.c_double(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    _lib.load().pixo_hip_debug_jpeg_entropy_last(C.byref(ms), C.byref(r), C.byref(d), C.byref(h))
    return dict(device_ms=ms.value, rounds=r.value, files_device=d.value, files_redone=h.value)
