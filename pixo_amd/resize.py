"""`pixo::resize` on the MI355X (reference src/resize.rs): nearest, bilinear and Lanczos3, byte for byte the reference's.
Mirrors `ResizeAlgorithm`, `ResizeOptions` and its builder, `resize`, `resize_into`, and the wasm export `resizeImage`
(src/wasm.rs:183-201) as `resize_image`.  No CPU fallback."""
import ctypes as C
import enum
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._images import bpp as _bpp, check_block, flat_u8, image_bytes, image_records, images_block, pair
from .color import ColorType

MAX_DIMENSION = 1 << 24

# this module's bits of the route record (pixo_hip_debug_routes; pixo_amd/csrc/routes.hpp)
ROUTES = {"RESIZE_NEAREST": 36, "RESIZE_BILINEAR": 37, "RESIZE_LANCZOS3": 38, "RESIZE_BATCH": 41, "RESIZE_IMAGES": 47}
ROUTE_RESIZE_NEAREST, ROUTE_RESIZE_BILINEAR, ROUTE_RESIZE_LANCZOS3, ROUTE_RESIZE_BATCH, ROUTE_RESIZE_IMAGES = (1 << b for b in ROUTES.values())


class ResizeAlgorithm(enum.IntEnum):
    Nearest = 0
    Bilinear = 1  # the default
    Lanczos3 = 2


@dataclass(frozen=True)
class ResizeOptions:
    src_width: int
    src_height: int
    dst_width: int
    dst_height: int
    color_type: ColorType = ColorType.Rgba
    algorithm: ResizeAlgorithm = ResizeAlgorithm.Bilinear

    @staticmethod
    def builder(src_width: int, src_height: int) -> "ResizeOptionsBuilder":
        return ResizeOptionsBuilder(src_width, src_height)

    def output_len(self) -> int:
        return self.dst_width * self.dst_height * ColorType(self.color_type).bytes_per_pixel()

    def _c(self) -> _lib.ResizeOptionsC:
        return _lib.ResizeOptionsC(self.src_width, self.src_height, self.dst_width, self.dst_height,
                                   int(self.color_type), int(self.algorithm))


class ResizeOptionsBuilder:
    """resize.rs:94-150: destination defaults to the source size, colour type to Rgba, algorithm to Bilinear."""

    def __init__(self, src_width: int, src_height: int):
        self._v = dict(src_width=src_width, src_height=src_height, dst_width=src_width, dst_height=src_height,
                       color_type=ColorType.Rgba, algorithm=ResizeAlgorithm.Bilinear)

    def dst(self, width: int, height: int) -> "ResizeOptionsBuilder":
        self._v.update(dst_width=width, dst_height=height)
        return self

    def color_type(self, color_type) -> "ResizeOptionsBuilder":
        self._v["color_type"] = ColorType(color_type)
        return self

    def algorithm(self, algorithm) -> "ResizeOptionsBuilder":
        self._v["algorithm"] = ResizeAlgorithm(algorithm)
        return self

    def build(self) -> ResizeOptions:
        return ResizeOptions(**self._v)


def resize(data, options: ResizeOptions) -> bytes:
    """Host pixels -> the resized pixels."""
    L = _lib.load()
    px = flat_u8(data)
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    o = options._c()
    rc = L.pixo_hip_resize(px.ctypes.data, px.size, C.byref(o), C.byref(out), C.byref(n))
    _lib.check(rc)
    return _lib.take(L, out, n)


def resize_into(output, data, options: ResizeOptions) -> int:
    """Writes into `output` (a writable uint8 numpy array); returns the bytes written.  BufferTooSmall carries the bytes
    needed in `.needed`."""
    L = _lib.load()
    px = flat_u8(data)
    assert output.dtype == np.uint8 and output.flags["C_CONTIGUOUS"] and output.flags["WRITEABLE"]
    n = C.c_size_t()
    o = options._c()
    rc = L.pixo_hip_resize_into(output.ctypes.data, output.nbytes, px.ctypes.data, px.size, C.byref(o), C.byref(n))
    _lib.check(rc, needed=n.value)
    return n.value


def resize_device(d_src, options: ResizeOptions, d_dst, stream=0) -> None:
    """Device pixels (torch tensor / raw pointer) -> d_dst.  Enqueue only: the kernels run on `stream` behind the work of the
    producer stream (jpeg.set_producer_stream)."""
    L = _lib.load()

    o = options._c()
    rc = L.pixo_hip_resize_device(_lib.ptr(d_src), C.byref(o), _lib.ptr(d_dst), C.c_void_p(stream) if stream else None)
    _lib.check(rc)


def _sources_c(sources, bpp, address):
    """(pixels, width, height) triples as the C array; whatever carries a size (tensor, array) must hold width * height * bpp bytes
    (the C entries take no length)."""
    arr = (_lib.ResizeSourceC * max(len(sources), 1))()
    for i, (px, w, h) in enumerate(sources):
        if bpp and (hasattr(px, "numel") or hasattr(px, "nbytes")):
            need, have = w * h * bpp, _lib.nbytes(px)
            if have != need:
                raise ValueError("source %d of %dx%d needs %d bytes of pixels, it holds %d" % (i, w, h, need, have))
        arr[i] = _lib.ResizeSourceC(address(px), w, h)
    return arr


def resize_batch_device(sources, dst_width, dst_height, color_type, algorithm, d_dst, stream=0) -> None:
    """`sources`: a list of (tensor_or_pointer, width, height) in HBM, each of its own size -> len(sources) images of
    dst_width x dst_height back to back at d_dst, image i byte for byte what `resize_device` writes for source i: the layout
    `jpeg.encode_batch_device` and `png.encode_batch_device` read.  One launch per pass whatever the number of images.
    Enqueue only, ordered like `resize_device`."""
    L = _lib.load()
    bpp = _bpp(color_type)
    arr = _sources_c(sources, bpp, _lib.ptr)
    if bpp and hasattr(d_dst, "numel"):
        need, have = len(sources) * dst_width * dst_height * bpp, _lib.nbytes(d_dst)
        if have != need:
            raise ValueError("a batch of %d images of %dx%d needs %d bytes of output, the tensor holds %d" % (len(sources), dst_width, dst_height, need, have))
    rc = L.pixo_hip_resize_batch_device(arr, len(sources), dst_width, dst_height, int(color_type), int(algorithm), _lib.ptr(d_dst),
                                        C.c_void_p(stream) if stream else None)
    _lib.check(rc)


def resize_batch(sources, dst_width, dst_height, color_type, algorithm) -> list:
    """Host pixels: a list of (pixels, width, height) -> a list of bytes, image i what `resize` makes of source i."""
    L = _lib.load()
    bpp = _bpp(color_type)
    held = [(flat_u8(px), w, h) for px, w, h in sources]
    arr = _sources_c(held, bpp, _lib.address)
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    rc = L.pixo_hip_resize_batch(arr, len(held), dst_width, dst_height, int(color_type), int(algorithm), C.byref(out), C.byref(n))
    _lib.check(rc)
    block, each = _lib.take(L, out, n), dst_width * dst_height * bpp
    return [block[i * each:(i + 1) * each] for i in range(len(held))]


def resize_batch_plan(sizes, dst_width, dst_height, color_type, algorithm) -> dict:
    """What the batch entries decide for sources of these (width, height), computed on the host (no GPU): `sub_first` (where
    each sub-batch starts, and the batch's end), `mid_at` (each image's offset in its sub-batch's Lanczos3 intermediate),
    `use_lds` (its horizontal pass stages in LDS) and `axis_tables` (distinct axis tables built)."""
    L = _lib.load()
    n = len(sizes)
    arr = (_lib.ResizeSourceC * max(n, 1))(*[_lib.ResizeSourceC(None, w, h) for w, h in sizes])
    sub_first, mid_at, use_lds = (C.c_uint32 * (n + 1))(), (C.c_uint64 * max(n, 1))(), (C.c_uint8 * max(n, 1))()
    subs, tables = C.c_uint32(), C.c_uint32()
    rc = L.pixo_hip_debug_resize_batch_plan(arr, n, dst_width, dst_height, int(color_type), int(algorithm), sub_first, C.byref(subs),
                                            mid_at, use_lds, C.byref(tables))
    _lib.check(rc)
    return dict(sub_first=list(sub_first[:subs.value + 1]), mid_at=list(mid_at[:n]), use_lds=[bool(v) for v in use_lds[:n]],
                axis_tables=tables.value)


# ---- images of individual sizes and colour types, anywhere in one block (include/pixo_hip.h) --------------------------------
# The records are the ones `decode.decode_png_batch_info` returns and `png.encode_images*` take: a `_lib.PngImageC` array, a list
# of (width, height, ColorType, offset), or the (tensor, ColorType) views of `decode.decode_png_batch_device`.
FIT_NO_ENLARGE = 1  # PIXO_RESIZE_FIT_NO_ENLARGE


def fit_images(images, box_width, box_height, no_enlarge=False):
    """([(width, height, ColorType, offset)], total): every image at the largest size of its proportions inside box_width x
    box_height (the reference front end's `calculateResizeDimensions`), in its own colour type, laid out as a decode batch
    lays its block out — every offset a multiple of 16, `total` the end of the last image.  `no_enlarge`: an image that fits
    the box keeps its size.  Sizes only: no GPU."""
    L = _lib.load()
    arr, n, _ = image_records(images)
    out, total = (_lib.PngImageC * max(n, 1))(), C.c_size_t()
    _lib.check(L.pixo_hip_resize_images_fit(arr, n, box_width, box_height, FIT_NO_ENLARGE if no_enlarge else 0, out, C.byref(total)))
    return [(im.width, im.height, ColorType(im.color_type), im.offset) for im in out[:n]], total.value


def resize_images_device(d_src, src_images, d_dst, dst_images, algorithm, stream=0) -> None:
    """Image i of `src_images` in the block `d_src` (torch tensor / raw pointer; None with the views of a decode batch, which
    carry their block) -> `dst_images[i]`'s size at its offset in `d_dst`, byte for byte what `resize_device` writes for that
    pair; the bytes between destinations are left as they are.  Destinations must not overlap each other or a source (not
    checked).  One launch per pass and pixel size whatever the number of images.  Enqueue only, ordered like `resize_device`."""
    L = _lib.load()
    src, dst, n, base = pair(src_images, dst_images)
    d_src = images_block(d_src, base)
    check_block("sources", d_src, src, n)
    check_block("destinations", d_dst, dst, n)
    rc = L.pixo_hip_resize_images_device(_lib.ptr(d_src), src, _lib.ptr(d_dst), dst, n, int(algorithm), C.c_void_p(stream) if stream else None)
    _lib.check(rc)


def resize_images(block_bytes, src_images, dst_images, algorithm) -> list:
    """The same for a block in host memory (what `decode.decode_png_batch` works from) -> a list of bytes, image i at
    `dst_images[i]`'s size."""
    L = _lib.load()
    src, dst, n, _ = pair(src_images, dst_images)
    px = flat_u8(block_bytes)
    out, out_len = C.POINTER(C.c_uint8)(), C.c_size_t()
    _lib.check(L.pixo_hip_resize_images(px.ctypes.data, px.size, src, dst, n, int(algorithm), C.byref(out), C.byref(out_len)))
    block = _lib.take(L, out, out_len)
    return [block[im.offset:im.offset + image_bytes(im)] for im in dst[:n]]


def resize_images_plan(src_images, dst_images, algorithm) -> dict:
    """What the images entries decide for these records, computed on the host (no GPU): `sub_first`, `mid_at`, `use_lds` and
    `axis_tables` as `resize_batch_plan`; `tiles_first` / `tiles_second` (each image's workgroups in the point or horizontal
    pass and in the vertical pass) and `launches_first` / `launches_second` (the passes' launches summed over the sub-batches)."""
    L = _lib.load()
    src, dst, n, _ = pair(src_images, dst_images)
    sub_first, mid_at, use_lds = (C.c_uint32 * (n + 1))(), (C.c_uint64 * max(n, 1))(), (C.c_uint8 * max(n, 1))()
    t1, t2 = (C.c_uint32 * max(n, 1))(), (C.c_uint32 * max(n, 1))()
    subs, tables, l1, l2 = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = L.pixo_hip_debug_resize_images_plan(src, dst, n, int(algorithm), sub_first, C.byref(subs), mid_at, use_lds, t1, t2, C.byref(tables),
                                             C.byref(l1), C.byref(l2))
    _lib.check(rc)
    return dict(sub_first=list(sub_first[:subs.value + 1]), mid_at=list(mid_at[:n]), use_lds=[bool(v) for v in use_lds[:n]],
                tiles_first=list(t1[:n]), tiles_second=list(t2[:n]), axis_tables=tables.value, launches_first=l1.value, launches_second=l2.value)


def resize_image(data, src_width, src_height, dst_width, dst_height, color_type: int, algorithm: int) -> bytes:
    """The wasm export `resizeImage`: seven flat arguments, its error strings."""
    L = _lib.load()
    px = flat_u8(data)
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    if not (0 <= color_type <= 255 and 0 <= algorithm <= 255):
        raise ValueError("color_type and algorithm are u8")
    rc = L.pixo_hip_resize_image(px.ctypes.data, px.size, src_width, src_height, dst_width, dst_height, color_type, algorithm,
                                 C.byref(out), C.byref(n))
    _lib.check(rc)
    return _lib.take(L, out, n)


def contributions(src: int, dst: int):
    """The Lanczos3 table of one axis, computed on the host (no GPU): (starts u32[dst], counts u32[dst], weights f32[total])."""
    L = _lib.load()
    total = C.c_size_t()
    rc = L.pixo_hip_resize_contributions(src, dst, None, None, None, 0, C.byref(total))
    if rc and rc != -9:
        _lib.check(rc)
    starts, counts = np.empty(dst, np.uint32), np.empty(dst, np.uint32)
    weights = np.empty(max(total.value, 1), np.float32)
    rc = L.pixo_hip_resize_contributions(src, dst, starts.ctypes.data, counts.ctypes.data, weights.ctypes.data, total.value, C.byref(total))
    _lib.check(rc)
    return starts, counts, weights[:total.value]
