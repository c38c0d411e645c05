"""What the modules that take `pixo_png_image` records share (png, jpeg, resize, convert, decode): the records themselves, the
block they lie in, and the sizes Python checks because the C entries take no length for a device block.  The records are the
ones `decode.decode_png_batch_info` returns: a `_lib.PngImageC` array, a list of (width, height, ColorType, offset), or the
(tensor, ColorType) views of `decode.decode_png_batch_device`."""
import ctypes as C

import numpy as np

from . import _lib


def bpp(color_type) -> int:
    """Bytes per pixel; 0 for a code that is no colour type (the library refuses it with its own message: no size to check)"""
    return int(color_type) + 1 if 0 <= int(color_type) <= 3 else 0


def flat_u8(data) -> np.ndarray:
    """Host bytes (bytes-like, or anything numpy takes) as one contiguous row of uint8"""
    return np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8).reshape(-1)


def image_records(images):
    """`images` as (a PngImageC array, its length, the tensor the offsets count from or None): a PngImageC array as it is; a
    list of (width, height, ColorType, offset) as `decode.decode_png_batch_info` returns; or the list of (tensor, ColorType)
    views `decode.decode_png_batch_device` returns, whose offsets are the tensors' addresses relative to the first."""
    if isinstance(images, C.Array) and getattr(images, "_type_", None) is _lib.PngImageC:
        return images, len(images), None
    n = len(images)
    arr = (_lib.PngImageC * max(n, 1))()
    base = None
    for i, im in enumerate(images):
        if len(im) == 2 and hasattr(im[0], "data_ptr"):
            t, ct = im
            if base is None:
                base = t
            at = t.data_ptr() - base.data_ptr()
            if at < 0:
                raise ValueError("image %d lies in front of the first: the offsets count from the first view" % i)
            arr[i].offset, arr[i].width, arr[i].height, arr[i].color_type = at, t.shape[1], t.shape[0], int(ct)
        else:
            w, h, ct, at = im
            arr[i].offset, arr[i].width, arr[i].height, arr[i].color_type = at, w, h, int(ct)
    return arr, n, base


def images_block(block, base):
    """(the views of a decode batch carry their block with them: the first view's address is the block's)"""
    if block is None:
        if base is None:
            raise ValueError("no block: pass the tensor the images' offsets count from")
        return base.data_ptr()  # (the first view says nothing of the block's size: the address alone)
    return block


def image_bytes(im) -> int:
    return im.width * im.height * bpp(im.color_type)


def records_end(arr, n) -> int:
    """Where the furthest image ends"""
    return max(arr[i].offset + image_bytes(arr[i]) for i in range(n)) if n else 0


def check_block(what, block, arr, n) -> None:
    """(the C entries take no length for a device block: whatever carries a size is checked here)"""
    if hasattr(block, "numel") and n and all(bpp(arr[i].color_type) for i in range(n)):
        need, have = records_end(arr, n), _lib.nbytes(block)
        if have < need:
            raise ValueError("the %s end at byte %d, the tensor holds %d" % (what, need, have))


def pair(src_images, dst_images):
    """(source records, destination records, their number, the tensor the sources' offsets count from or None)"""
    src, n, base = image_records(src_images)
    dst, m, _ = image_records(dst_images)
    if m != n:
        raise ValueError("%d sources, %d destinations" % (n, m))
    return src, dst, n, base
