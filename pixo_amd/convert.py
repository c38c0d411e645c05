"""Colour conversion on the device: what the reference's front end does between a decode and an encode (src/bin/pixo.rs:478-513,
619-638) — drop the alpha channel in front of a JPEG, or go gray — for one image or for N images of individual sizes and
colour types in one pass, on pixels that stay in HBM.  The contract of every entry: include/pixo_hip.h.

    views = decode.decode_png_batch_device(files)                     # every image in its own colour type
    fitted, total = resize.fit_images(views, 256, 256)
    resize.resize_images_device(None, views, d_small, fitted, resize.ResizeAlgorithm.Lanczos3)
    opaque, total = convert.layout_images(fitted, convert.Target.OPAQUE)
    convert.convert_images_device(d_small, fitted, d_opaque, opaque)  # Rgba -> Rgb, GrayAlpha -> Gray, the rest copied
    files = jpeg.encode_images_device(d_opaque, opaque, options)
"""
import ctypes as C
import enum

from . import _lib
from ._images import bpp, check_block, flat_u8, image_bytes, image_records, images_block, pair
from .color import ColorType


class Target(enum.IntEnum):
    """What a batch is converted to: OPAQUE (GrayAlpha -> Gray, Rgba -> Rgb, Gray and Rgb kept: what a JPEG takes) or GRAY
    (everything -> Gray: the front end's --grayscale)."""
    OPAQUE = 0
    GRAY = 1


KINDS = ("copy", "gray_alpha_to_gray", "rgba_to_rgb", "rgb_to_gray", "rgba_to_gray")  # the plan's kind[i]
FORMS = ("aligned", "bytes")  # ... and form[i]


def tile_pixels() -> int:
    """Pixels one workgroup of the conversion kernels takes in a step (tests place their sizes by it)."""
    return _lib.load().pixo_hip_debug_convert_tile_pixels()


def layout_images(images, target):
    """([(width, height, ColorType, offset)], total): every image at its own size in the colour type `target` gives it, laid
    out as a decode batch lays its block out — every offset a multiple of 16, `total` the end of the last image.  Sizes
    only: no GPU."""
    L = _lib.load()
    arr, n, _ = image_records(images)
    out, total = (_lib.PngImageC * max(n, 1))(), C.c_size_t()
    _lib.check(L.pixo_hip_convert_images_layout(arr, n, int(target), out, C.byref(total)))
    return [(im.width, im.height, ColorType(im.color_type), im.offset) for im in out[:n]], total.value


def convert_images_device(d_src, src_images, d_dst, dst_images, stream=0) -> None:
    """Image i of `src_images` in the block `d_src` (torch tensor / raw pointer; None with the views of a decode batch, which
    carry their block) -> the same pixels in `dst_images[i]`'s colour type at its offset in `d_dst`, byte for byte what
    `convert_device` writes for that image; the bytes between destinations are left as they are.  Destinations must not
    overlap each other or a source (not checked).  One launch per conversion present and alignment class, whatever the number
    of images.  Enqueue only, ordered like `resize.resize_images_device`."""
    L = _lib.load()
    src, dst, n, base = pair(src_images, dst_images)
    d_src = images_block(d_src, base)
    check_block("sources", d_src, src, n)
    check_block("destinations", d_dst, dst, n)
    _lib.check(L.pixo_hip_convert_images_device(_lib.ptr(d_src), src, _lib.ptr(d_dst), dst, n, C.c_void_p(stream) if stream else None))


def convert_images(block_bytes, src_images, dst_images) -> list:
    """The same for a block in host memory -> a list of bytes, image i in `dst_images[i]`'s colour type."""
    L = _lib.load()
    src, dst, n, _ = pair(src_images, dst_images)
    px = flat_u8(block_bytes)
    out, out_len = C.POINTER(C.c_uint8)(), C.c_size_t()
    _lib.check(L.pixo_hip_convert_images(px.ctypes.data, px.size, src, dst, n, C.byref(out), C.byref(out_len)))
    block = _lib.take(L, out, out_len)
    return [block[im.offset:im.offset + image_bytes(im)] for im in dst[:n]]


def convert_images_plan(src_images, dst_images, src_align=0, dst_align=0) -> dict:
    """What `convert_images_device` decides for these records when its blocks' addresses are `src_align` and `dst_align`
    modulo 16, computed on the host (no GPU): `sub_first` (where each sub-batch starts, and the batch's end), per image
    `kind` (an index into KINDS), `form` (into FORMS) and `tiles` (its workgroups), and `launches` (summed over the
    sub-batches)."""
    L = _lib.load()
    src, dst, n, _ = pair(src_images, dst_images)
    sub_first, subs, launches = (C.c_uint32 * (n + 1))(), C.c_uint32(), C.c_uint32()
    kind, form, tiles = (C.c_uint8 * max(n, 1))(), (C.c_uint8 * max(n, 1))(), (C.c_uint32 * max(n, 1))()
    _lib.check(L.pixo_hip_debug_convert_images_plan(src, dst, n, src_align, dst_align, sub_first, C.byref(subs), kind, form, tiles, C.byref(launches)))
    return dict(sub_first=list(sub_first[:subs.value + 1]), kind=list(kind[:n]), form=list(form[:n]), tiles=list(tiles[:n]), launches=launches.value)


def convert_device(d_src, width, height, src_color_type, dst_color_type, d_dst, stream=0) -> None:
    """width x height pixels of `src_color_type` at d_src -> `dst_color_type` at d_dst (torch tensors / raw pointers in HBM,
    any alignment).  Enqueue only, ordered like `resize.resize_device`."""
    L = _lib.load()
    for what, block, ct in (("source", d_src, src_color_type), ("destination", d_dst, dst_color_type)):
        if hasattr(block, "numel") and bpp(ct):
            need, have = width * height * bpp(ct), _lib.nbytes(block)
            if have < need:
                raise ValueError("the %s needs %d bytes, the tensor holds %d" % (what, need, have))
    _lib.check(L.pixo_hip_convert_device(_lib.ptr(d_src), width, height, int(src_color_type), int(dst_color_type), _lib.ptr(d_dst),
                                         C.c_void_p(stream) if stream else None))


def convert(data, width, height, src_color_type, dst_color_type) -> bytes:
    """Host pixels -> the converted pixels (bytes)."""
    L = _lib.load()
    px = flat_u8(data)
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    _lib.check(L.pixo_hip_convert(px.ctypes.data, px.size, width, height, int(src_color_type), int(dst_color_type), C.byref(out), C.byref(n)))
    return _lib.take(L, out, n)


# ---- the reference front end's three functions (src/bin/pixo.rs:478-513): flat pixel data of any length ----------------------
def _run(data, src_ct, dst_ct) -> bytes:
    px = flat_u8(data)
    size = bpp(src_ct)
    if px.size % size:
        raise ValueError("%d bytes are no whole number of %d-byte pixels" % (px.size, size))
    pixels = px.size // size
    if pixels == 0:
        return b""
    # (a run of pixels is an image of one row, or of rows of 2^24 with the last pixels in a call of their own)
    side, out = 1 << 24, []
    whole = pixels // side
    if whole:
        out.append(convert(px[:whole * side * size], side, whole, src_ct, dst_ct))
    if pixels % side:
        out.append(convert(px[whole * side * size:], pixels % side, 1, src_ct, dst_ct))
    return b"".join(out)


def gray_alpha_to_gray(data) -> bytes:
    return _run(data, ColorType.GrayAlpha, ColorType.Gray)


def rgba_to_rgb(data) -> bytes:
    return _run(data, ColorType.Rgba, ColorType.Rgb)


def to_grayscale(data, color_type) -> bytes:
    return _run(data, color_type, ColorType.Gray)
