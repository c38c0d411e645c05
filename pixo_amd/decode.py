"""`pixo::decode` on the MI355X (reference src/decode/png.rs): a PNG file -> 8-bit pixels.  The chunk walk, its checks and the
inflate run on the host, in the reference's order and with its messages; row reconstruction and the conversion to pixels run
on the device.  Mirrors `PngImage` and `decode_png`; `decode_png_info` and `decode_png_device` are what a caller needs to keep
the pixels in device memory for `resize.resize_device`, `jpeg.encode_device` and `png.encode_device`.  JPEG decode is not
provided.  No CPU fallback."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .color import ColorType


@dataclass(frozen=True)
class PngImage:
    """png.rs:18-28"""
    width: int
    height: int
    pixels: bytes
    color_type: ColorType


def _file(data) -> np.ndarray:
    return np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8).reshape(-1)


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


def inflate_zlib(data, expected: int) -> bytes:
    """The host inflate alone (inflate.rs:294-352 with Some(expected)); no GPU."""
    L = _lib.load()
    f = _file(data)
    out = np.empty(max(expected, 1), np.uint8)
    _lib.check(L.pixo_hip_zlib_inflate(f.ctypes.data if f.size else out.ctypes.data, f.size, out.ctypes.data, expected))
    return out[:expected].tobytes()
