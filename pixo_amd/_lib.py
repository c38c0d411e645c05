"""Loader for the C-ABI library (pixo_amd/libpixo_hip.so, built by pixo_amd/csrc/Makefile).

There is no CPU fallback: if the HIP library is missing, importing the compute entry
points fails loudly.
"""
import ctypes as C
import os

from .error import BufferTooSmall, from_status

_HERE = os.path.dirname(os.path.abspath(__file__))
# PIXO_HIP_LIB lets kernel A/B experiments (tools/ab_build.sh) point at another build of the
# same C ABI; the default is the in-tree library.
LIB_PATH = os.environ.get("PIXO_HIP_LIB") or os.path.join(_HERE, "libpixo_hip.so")


class JpegOptionsC(C.Structure):
    """pixo_jpeg_options (include/pixo_hip.h)"""
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("color_type", C.c_uint8), ("quality", C.c_uint8), ("subsampling", C.c_uint8),
        ("has_restart_interval", C.c_uint8), ("restart_interval", C.c_uint16),
        ("optimize_huffman", C.c_uint8), ("progressive", C.c_uint8), ("trellis_quant", C.c_uint8),
    ]


class ResizeOptionsC(C.Structure):
    """pixo_resize_options (include/pixo_hip.h)"""
    _fields_ = [
        ("src_width", C.c_uint32), ("src_height", C.c_uint32), ("dst_width", C.c_uint32), ("dst_height", C.c_uint32),
        ("color_type", C.c_uint8), ("algorithm", C.c_uint8),
    ]


class ResizeSourceC(C.Structure):
    """pixo_resize_source (include/pixo_hip.h): one source of a resize batch"""
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32)]


class PngFileC(C.Structure):
    """pixo_png_file (include/pixo_hip.h): one file of a decode batch"""
    _fields_ = [("data", C.c_void_p), ("len", C.c_size_t)]


class PngImageC(C.Structure):
    """pixo_png_image (include/pixo_hip.h): one image of the block a decode batch writes"""
    _fields_ = [("offset", C.c_uint64), ("width", C.c_uint32), ("height", C.c_uint32), ("color_type", C.c_uint8), ("reserved", C.c_uint8 * 7)]


class PngOptionsC(C.Structure):
    """pixo_png_options (include/pixo_hip.h)"""
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("color_type", C.c_uint8), ("filter_strategy", C.c_uint8), ("optimize_alpha", C.c_uint8),
        ("reduce_color_type", C.c_uint8), ("reduce_palette", C.c_uint8), ("compression_level", C.c_uint8),
        ("optimal_compression", C.c_uint8), ("strip_metadata", C.c_uint8), ("flags", C.c_uint32),
    ]


class PngLayoutC(C.Structure):
    """pixo_png_layout (include/pixo_hip.h)"""
    _fields_ = [
        ("color_type_byte", C.c_uint8), ("bit_depth", C.c_uint8), ("bytes_per_pixel", C.c_uint8), ("has_trns", C.c_uint8),
        ("row_bytes", C.c_uint32), ("palette_len", C.c_uint32), ("palette", (C.c_uint8 * 4) * 256),
    ]


class PngQuantizationC(C.Structure):
    """pixo_png_quantization (include/pixo_hip.h)"""
    _fields_ = [("mode", C.c_uint8), ("dithering", C.c_uint8), ("max_colors", C.c_uint16)]


def _sig(*argtypes, ret=C.c_int, optional=False):
    """One row of SIGNATURES.  No argtypes: left unset (the entry takes none, or ctypes' defaults serve).  optional: absent
    from the older builds that A/B timing loads through PIXO_HIP_LIB (tools/ab/)."""
    return (list(argtypes) or None, ret, optional)


_vp, _sz, _u8, _u32, _u64, _int, _dbl = C.c_void_p, C.c_size_t, C.c_uint8, C.c_uint32, C.c_uint64, C.c_int, C.c_double
_szp, _u8p, _u32p, _u64p, _i16p = C.POINTER(_sz), C.POINTER(_u8), C.POINTER(_u32), C.POINTER(_u64), C.POINTER(C.c_int16)
_u8pp, _optp, _roptp = C.POINTER(_u8p), C.POINTER(JpegOptionsC), C.POINTER(ResizeOptionsC)
_poptp, _playp, _qoptp = C.POINTER(PngOptionsC), C.POINTER(PngLayoutC), C.POINTER(PngQuantizationC)
_rsrcp = C.POINTER(ResizeSourceC)
_pfilep, _pimgp = C.POINTER(PngFileC), C.POINTER(PngImageC)
_coeffs = (_vp, _u32, _u32, _u8, _u8, _u8, _vp, _sz, _vp, _vp, _sz)

# every symbol include/pixo_hip.h declares: name -> (argtypes, restype, optional).  `load()` applies it; a new entry is declared
# there and here (tests/test_cabi_cpu.py holds the two against each other).
SIGNATURES = {
    "pixo_jpeg_options_from_preset": _sig(_optp, _u32, _u32, _u8, _u8, ret=None),
    "pixo_hip_jpeg_encode": _sig(_vp, _sz, _optp, _u8pp, _szp),
    "pixo_hip_jpeg_encode_into": _sig(_vp, _sz, _vp, _sz, _optp, _szp),
    "pixo_hip_encode_jpeg": _sig(_vp, _sz, _u32, _u32, _u8, _u8, _u8, _int, _u8pp, _szp),
    "pixo_hip_coeff_geometry": _sig(_u32, _u32, _u8, _u8, _szp, _szp),
    "pixo_hip_jpeg_coeffs": _sig(*_coeffs),
    "pixo_hip_jpeg_coeffs_device": _sig(_vp, _u32, _u32, _u8, _u8, _u8, _u32, _vp, _vp, _vp, _vp),
    "pixo_hip_jpeg_coeffs_integer": _sig(*_coeffs),
    "pixo_hip_jpeg_coeffs_integer_device": _sig(_vp, _u32, _u32, _u8, _u8, _u8, _vp, _vp, _vp, _vp),
    "pixo_hip_jpeg_entropy_encode": _sig(_vp, _vp, _vp, _optp, _u8pp, _szp),
    "pixo_hip_jpeg_entropy_encode_device": _sig(_vp, _vp, _vp, _optp, _u8pp, _szp),
    "pixo_hip_jpeg_encode_device": _sig(_vp, _optp, _u8pp, _szp),
    "pixo_hip_jpeg_encode_device_into": _sig(_vp, _optp, _vp, _sz, _szp),
    "pixo_hip_jpeg_encode_batch_device": _sig(_vp, _optp, _u32, _u8pp, _szp),
    "pixo_hip_jpeg_encode_batch_device_into": _sig(_vp, _optp, _u32, _vp, _sz, _szp, _szp),
    "pixo_hip_jpeg_encode_images_device": _sig(_vp, _pimgp, _u32, _optp, _u8pp, _szp, optional=True),
    "pixo_hip_jpeg_encode_images_device_into": _sig(_vp, _pimgp, _u32, _optp, _vp, _sz, _szp, _szp, optional=True),
    "pixo_hip_jpeg_encode_images": _sig(_vp, _sz, _pimgp, _u32, _optp, _u8pp, _szp, optional=True),
    "pixo_hip_debug_jpeg_encode_images_plan": _sig(_pimgp, _u32, _optp, _u32, _u32p, _u32p, _u8p, _u8p, _u64p, _u32p, _u32p, optional=True),
    "pixo_hip_debug_lookback_fallbacks": _sig(ret=_u64),
    "pixo_hip_debug_routes": _sig(_int, ret=_u64, optional=True),
    "pixo_hip_debug_dispatch_gate": _sig(_u64p, _u64p, optional=True),
    "pixo_hip_debug_stream_copy": _sig(_vp, _vp, _sz, _vp),
    "pixo_hip_debug_stream_io": _sig(_vp, _vp, _u32, _u32, _u32, _vp, optional=True),
    "pixo_hip_debug_engine_clock": _sig(_vp, C.POINTER(_dbl), optional=True),
    "pixo_hip_debug_scan_device_async": _sig(_vp, _optp, _vp, C.POINTER(_int)),
    "pixo_hip_debug_scan_device_async_batch": _sig(_vp, _optp, _u32, _vp, C.POINTER(_int), optional=True),
    "pixo_hip_png_filter": _sig(_vp, _sz, _u32, _u32, _u32, _u8, _u32, _vp, _sz, _u32p),
    "pixo_hip_png_filter_device": _sig(_vp, _u32, _u32, _u32, _u8, _u32, _vp, _u32p),
    "pixo_hip_png_filter_async": _sig(_vp, _u32, _u32, _u32, _u8, _u32, _vp, _vp, _vp, _vp),
    "pixo_hip_png_adler32_from_row_sums": _sig(_vp, _u32, _u32, _u32, ret=_u32),
    "pixo_hip_png_options_from_preset": _sig(_poptp, _u32, _u32, _u8, ret=None),
    "pixo_hip_png_prepare": _sig(_vp, _sz, _poptp, _vp, _sz, _szp, _playp, _u32p),
    "pixo_hip_png_prepare_device": _sig(_vp, _poptp, _vp, _playp, _szp, _u32p),
    "pixo_hip_png_palette_order": _sig(_vp, _vp, _u32, _vp),
    "pixo_hip_zlib_compress": _sig(_vp, _sz, _u8, _u32, _u32, _u8pp, _szp),
    "pixo_hip_zlib_compress_device": _sig(_vp, _sz, _u8, _u32, _u32, _vp, _sz, _szp),
    "pixo_hip_zlib_compress_effort": _sig(_vp, _sz, _u8, _u32, _u32, _u32, _u8pp, _szp, optional=True),
    "pixo_hip_zlib_compress_effort_device": _sig(_vp, _sz, _u8, _u32, _u32, _u32, _vp, _sz, _szp, optional=True),
    "pixo_hip_png_deflate_effort_params": _sig(_u32p, _u32p, ret=None, optional=True),
    "pixo_hip_png_encode": _sig(_vp, _sz, _poptp, _u8pp, _szp),
    "pixo_hip_png_encode_device": _sig(_vp, _poptp, _u8pp, _szp),
    "pixo_hip_png_quantize": _sig(_vp, _sz, _poptp, _qoptp, _vp, _sz, _vp, _u32p, _u32p, _u8p),
    "pixo_hip_png_quantize_device": _sig(_vp, _poptp, _qoptp, _vp, _vp, _u32p, _u32p, _u8p),
    "pixo_hip_png_encode_lossy": _sig(_vp, _sz, _poptp, _qoptp, _u8pp, _szp),
    "pixo_hip_png_encode_lossy_device": _sig(_vp, _poptp, _qoptp, _u8pp, _szp),
    "pixo_hip_png_encode_batch_device": _sig(_vp, _poptp, _qoptp, _u32, _u8pp, _szp, optional=True),
    "pixo_hip_png_encode_batch_device_into": _sig(_vp, _poptp, _qoptp, _u32, _vp, _sz, _szp, _szp, optional=True),
    "pixo_hip_png_encode_batch": _sig(_vp, _sz, _poptp, _qoptp, _u32, _u8pp, _szp, optional=True),
    "pixo_hip_debug_png_dither_stats": _sig(_u64p, _u64p, _u64p),
    "pixo_hip_png_median_cut": _sig(_vp, _vp, _u32, _u32, _vp, _u32p),
    "pixo_hip_resize": _sig(_vp, _sz, _roptp, _u8pp, _szp),
    "pixo_hip_resize_into": _sig(_vp, _sz, _vp, _sz, _roptp, _szp),
    "pixo_hip_resize_device": _sig(_vp, _roptp, _vp, _vp),
    "pixo_hip_resize_image": _sig(_vp, _sz, _u32, _u32, _u32, _u32, _u8, _u8, _u8pp, _szp),
    "pixo_hip_resize_contributions": _sig(_u32, _u32, _vp, _vp, _vp, _sz, _szp),
    "pixo_hip_resize_batch_device": _sig(_rsrcp, _u32, _u32, _u32, _u8, _u8, _vp, _vp, optional=True),
    "pixo_hip_resize_batch": _sig(_rsrcp, _u32, _u32, _u32, _u8, _u8, _u8pp, _szp, optional=True),
    "pixo_hip_debug_resize_batch_plan": _sig(_rsrcp, _u32, _u32, _u32, _u8, _u8, _u32p, _u32p, _u64p, _u8p, _u32p, optional=True),
    "pixo_hip_resize_images_fit": _sig(_pimgp, _u32, _u32, _u32, _u32, _pimgp, _szp, optional=True),
    "pixo_hip_resize_images_device": _sig(_vp, _pimgp, _vp, _pimgp, _u32, _u8, _vp, optional=True),
    "pixo_hip_resize_images": _sig(_vp, _sz, _pimgp, _pimgp, _u32, _u8, _u8pp, _szp, optional=True),
    "pixo_hip_debug_resize_images_plan": _sig(_pimgp, _pimgp, _u32, _u8, _u32p, _u32p, _u64p, _u8p, _u32p, _u32p, _u32p, _u32p, _u32p, optional=True),
    "pixo_hip_convert_images_layout": _sig(_pimgp, _u32, _u8, _pimgp, _szp, optional=True),
    "pixo_hip_convert_images_device": _sig(_vp, _pimgp, _vp, _pimgp, _u32, _vp, optional=True),
    "pixo_hip_convert_images": _sig(_vp, _sz, _pimgp, _pimgp, _u32, _u8pp, _szp, optional=True),
    "pixo_hip_convert_device": _sig(_vp, _u32, _u32, _u8, _u8, _vp, _vp, optional=True),
    "pixo_hip_convert": _sig(_vp, _sz, _u32, _u32, _u8, _u8, _u8pp, _szp, optional=True),
    "pixo_hip_debug_convert_images_plan": _sig(_pimgp, _pimgp, _u32, _u32, _u32, _u32p, _u32p, _u8p, _u8p, _u32p, _u32p, optional=True),
    "pixo_hip_debug_convert_tile_pixels": _sig(ret=_u32, optional=True),
    "pixo_hip_png_decode": _sig(_vp, _sz, _u8pp, _szp, _u32p, _u32p, _u8p),
    "pixo_hip_png_decode_info": _sig(_vp, _sz, _u32p, _u32p, _u8p),
    "pixo_hip_png_decode_device": _sig(_vp, _sz, _vp, _sz, _u32p, _u32p, _u8p, _vp),
    "pixo_hip_zlib_inflate": _sig(_vp, _sz, _vp, _sz),
    "pixo_hip_png_unfilter_pass_rows": _sig(ret=_u32),
    "pixo_hip_debug_png_decode_timed": _sig(_vp, _sz, C.POINTER(_dbl), _u64p),
    "pixo_hip_png_decode_batch_info": _sig(_pfilep, _u32, _pimgp, _szp, optional=True),
    "pixo_hip_png_decode_batch_device": _sig(_pfilep, _u32, _u32, _vp, _sz, _pimgp, _vp, optional=True),
    "pixo_hip_png_decode_batch": _sig(_pfilep, _u32, _u32, _u8pp, _szp, _pimgp, optional=True),
    "pixo_hip_debug_png_decode_batch_plan": _sig(_pfilep, _u32, _u32, _u32p, _u32p, _u64p, _u32p, _u32p, _u32p, optional=True),
    "pixo_hip_debug_png_decode_batch_timed": _sig(_pfilep, _u32, _u32, C.POINTER(_dbl), optional=True),
    "pixo_hip_jpeg_decode": _sig(_vp, _sz, _u8pp, _szp, _u32p, _u32p, _u8p, optional=True),
    "pixo_hip_jpeg_decode_info": _sig(_vp, _sz, _u32p, _u32p, _u8p, optional=True),
    "pixo_hip_jpeg_decode_device": _sig(_vp, _sz, _vp, _sz, _u32p, _u32p, _u8p, _vp, optional=True),
    "pixo_hip_jpeg_decode_batch_info": _sig(_pfilep, _u32, _pimgp, _szp, optional=True),
    "pixo_hip_jpeg_decode_batch_device": _sig(_pfilep, _u32, _u32, _vp, _sz, _pimgp, _vp, optional=True),
    "pixo_hip_jpeg_decode_batch": _sig(_pfilep, _u32, _u32, _u8pp, _szp, _pimgp, optional=True),
    "pixo_hip_debug_jpeg_decode_batch_plan": _sig(_pfilep, _u32, _u32, _u32p, _u32p, _u8p, _u32p, _u32p, optional=True),
    "pixo_hip_debug_jpeg_decode_batch_tables": _sig(_pfilep, _u32, _vp, optional=True),
    "pixo_hip_debug_jpeg_decode_coefficients": _sig(_vp, _sz, _u32, _vp, _sz, _u32p, _u32p, optional=True),
    "pixo_hip_jpeg_decode_tile_mcus": _sig(_u32p, _u32p, ret=None, optional=True),
    "pixo_hip_debug_jpeg_decode_batch_timed": _sig(_pfilep, _u32, _u32, C.POINTER(_dbl), optional=True),
    "pixo_hip_jpeg_entropy_geometry": _sig(_u32p, _u32p, _u32p, _u32p, ret=None, optional=True),
    "pixo_hip_debug_jpeg_entropy_plan": _sig(_pfilep, _u32, _u32, _u8p, _u32p, _u32p, optional=True),
    "pixo_hip_debug_jpeg_entropy_batch": _sig(_pfilep, _u32, _u32, _u32, _vp, _u64p, _u32p, optional=True),
    "pixo_hip_debug_jpeg_entropy_last": _sig(C.POINTER(_dbl), _u32p, _u32p, _u32p, ret=None, optional=True),
    "pixo_hip_png_encode_images_device": _sig(_vp, _pimgp, _u32, _poptp, _qoptp, _u8pp, _szp, optional=True),
    "pixo_hip_png_encode_images_device_into": _sig(_vp, _pimgp, _u32, _poptp, _qoptp, _vp, _sz, _szp, _szp, optional=True),
    "pixo_hip_png_encode_images": _sig(_vp, _sz, _pimgp, _u32, _poptp, _qoptp, _u8pp, _szp, optional=True),
    "pixo_hip_debug_png_encode_images_plan": _sig(_pimgp, _u32, _poptp, _qoptp, _u32, _u32p, _u32p, _u8p, _u8p, _u32p, optional=True),
    "pixo_hip_png_inflate_step_tokens":_sig(ret=_u32, optional=True),
    "pixo_hip_png_inflate_window_bytes": _sig(ret=_u32, optional=True),
    "pixo_hip_png_inflate_far_distance": _sig(ret=_u32, optional=True),
    "pixo_hip_png_inflate_stored_chunk": _sig(ret=_u32, optional=True),
    "pixo_hip_debug_zlib_inflate_batch_device": _sig(_pfilep, _u32, _u64p, _vp, _u64p, _u32p, _u64p, _u32p, C.POINTER(_dbl), optional=True),
    "pixo_hip_band": _sig(_u32, _u32, _u8, _u8, _u32, _u32, _u32p, _u32p, _szp, _szp, _szp, _szp),
    "pixo_hip_band_encoder_create": _sig(_optp, _u32, _u32, _int, C.POINTER(_vp)),
    "pixo_hip_band_encoder_destroy": _sig(_vp, ret=None),
    "pixo_hip_band_encoder_rows": _sig(_vp, _u32p, _u32p),
    "pixo_hip_band_encoder_coeffs": _sig(_vp, _vp, _int, _i16p),
    "pixo_hip_band_encoder_count": _sig(_vp, _i16p, _u64p),
    "pixo_hip_band_encoder_lengths": _sig(_vp, _i16p, _u64p, _u64p),
    "pixo_hip_band_encoder_pack": _sig(_vp, _u64, _u8pp, _szp),
    "pixo_hip_band_encoder_pack_device": _sig(_vp, _u64, _vp, C.POINTER(_vp), _szp),
    "pixo_hip_band_encoder_copy_body": _sig(_vp, _vp),
    "pixo_hip_jpeg_splice": _sig(_optp, _u64p, C.POINTER(_vp), _szp, _u32, _u8pp, _szp),
    "pixo_hip_jpeg_splice_layout": _sig(_optp, _u64p, _vp, _u32, _szp, _szp),
    "pixo_hip_jpeg_splice_finish": _sig(_optp, _u64p, _vp, _u32, _vp, _sz),
    "pixo_hip_jpeg_band_count_host": _sig(_vp, _vp, _vp, _optp, _u32, _i16p, _u64p),
    "pixo_hip_jpeg_band_bits_host": _sig(_vp, _vp, _vp, _optp, _u32, _i16p, _u64p, _u64p),
    "pixo_hip_jpeg_band_piece_host": _sig(_vp, _vp, _vp, _optp, _u32, _i16p, _u64p, _u64, _u8pp, _szp),
    "pixo_hip_jpeg_encode_multi": _sig(_vp, _sz, _optp, C.POINTER(_int), _u32, _u8pp, _szp),
    "pixo_hip_jpeg_encode_batch_multi": _sig(_vp, _optp, _u32, C.POINTER(_int), _u32, _vp, _sz, _szp, _szp),
    "pixo_hip_device_count": _sig(),
    "pixo_hip_set_device": _sig(_int),
    "pixo_hip_set_producer_stream": _sig(_vp),
    "pixo_hip_get_producer_stream": _sig(ret=_vp),
    "pixo_hip_debug_configure": _sig(C.c_char_p),
    "pixo_hip_trim": _sig(),
    "pixo_hip_free": _sig(_vp, ret=None),
    "pixo_hip_copy_file": _sig(_vp, _vp, _sz, ret=None),
    "pixo_hip_last_error": _sig(ret=C.c_char_p),
    "pixo_hip_version": _sig(ret=C.c_char_p),
}
SYMBOLS = list(SIGNATURES)

_lib = None


def _preload_process_hip_runtime():
    """One HIP runtime per process.  libpixo_hip.so needs `libamdhip64.so.7`; PyTorch-ROCm
    wheels bundle their own copy under torch/lib with the same soname.  Whichever is mapped
    first serves both, and mapping ROCm's first makes a later `import torch` find no GPU.
    So when torch is installed, map ITS runtime before ours (without importing torch)."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass  # fall back to the loader's default resolution (RUNPATH -> /opt/rocm/lib)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "pixo_amd: %s is missing — build it with `make -C pixo_amd/csrc` "
            "(or python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU fallback." % LIB_PATH)
    _preload_process_hip_runtime()
    L = C.CDLL(LIB_PATH)
    for name, (argtypes, restype, optional) in SIGNATURES.items():
        if optional and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    _lib = L
    return L


_bytes_new = C.pythonapi.PyBytes_FromStringAndSize
_bytes_new.restype = C.py_object
_bytes_new.argtypes = [C.c_void_p, C.c_ssize_t]


def file_bytes(L, ptr, n: int) -> bytes:
    """The n bytes at ptr as a Python bytes object.  Large files are copied by the library's copy threads into a bytes
    object created uninitialised (ours alone until it is returned), with a huge-page hint before its first touch:
    ctypes.string_at on a 178 MB file is a one-thread memcpy into 43,000 fresh pages, 28 ms of a 45 ms call."""
    if n < (2 << 20):
        return C.string_at(ptr, n)
    b = _bytes_new(None, n)
    L.pixo_hip_copy_file(C.cast(C.c_char_p(b), C.c_void_p), ptr, n)
    return b


def ptr(x):
    """A device address: that of a torch tensor, or the raw pointer itself."""
    return x.data_ptr() if hasattr(x, "data_ptr") else int(x)


def address(x):
    """Where a buffer starts: a torch tensor, a numpy array, or the raw address itself."""
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data if hasattr(x, "ctypes") else int(x)


def nbytes(x):
    """The capacity in bytes of a torch tensor or a numpy array."""
    return x.numel() * x.element_size() if hasattr(x, "numel") else x.nbytes


def check(rc, needed=None):
    """A status other than PIXO_OK raises the error it stands for (error.py), with the library's message; a BufferTooSmall
    carries `needed`, when the caller has it, as `.needed`: the bytes a second attempt has to bring."""
    if rc:
        e = from_status(rc, load().pixo_hip_last_error().decode())
        if needed is not None and isinstance(e, BufferTooSmall):
            e.needed = needed
        raise e


def take(L, p, n) -> bytes:
    """The block of n (a c_size_t) bytes the library handed over, as bytes; the block goes back to the library."""
    try:
        return file_bytes(L, p, n.value)
    finally:
        L.pixo_hip_free(p)


def take_files(L, files, lens, batch):
    """The `batch` blocks a batch entry handed over, as a list of bytes; every block goes back to the library, also when
    copying one of them raises."""
    try:
        return [file_bytes(L, files[i], lens[i]) for i in range(batch)]
    finally:
        for i in range(batch):
            L.pixo_hip_free(files[i])


def into_arena(entry, arena, batch):
    """The tail of the batch entries that write their files back to back into the caller's arena: a torch CPU tensor, a numpy
    array, or None for a size query.  `entry(address, capacity in bytes, offsets, lens)` makes the C call and returns its
    status.  Returns (offsets, lens) — of a size query too; files that do not fit raise BufferTooSmall with `.needed`,
    `.offsets` and `.lens`, which the library filled in all the same."""
    offsets, lens = (C.c_size_t * batch)(), (C.c_size_t * batch)()
    rc = entry(None, 0, offsets, lens) if arena is None else entry(address(arena), nbytes(arena), offsets, lens)
    if not (rc == -9 and arena is None):  # (PIXO_ERR_BUFFER_TOO_SMALL is the answer to a size query)
        try:
            check(rc, needed=int(offsets[batch - 1] + lens[batch - 1]) if batch else 0)
        except BufferTooSmall as e:
            e.offsets, e.lens = list(offsets), list(lens)
            raise
    return list(offsets), list(lens)
