"""PNG on the MI355X: row filters + Adler-32, the reductions in front of them, whole files —
`encode` compresses the prepared stream on the device and returns a finished PNG — and the lossy mode:
palette quantisation and Floyd-Steinberg dithering on the device.  Mirrors `pixo::png` (src/png/mod.rs).
No CPU fallback."""
import ctypes as C
import enum

import numpy as np

from . import _lib
from ._images import check_block, flat_u8, image_records, images_block
from .color import ColorType


class FilterStrategy(enum.IntEnum):
    NONE = 0
    SUB = 1
    UP = 2
    AVERAGE = 3
    PAETH = 4
    MINSUM = 5
    ADAPTIVE = 6
    ADAPTIVE_FAST = 7
    BIGRAMS = 8


# this module's bits of the route record (pixo_hip_debug_routes; pixo_amd/csrc/routes.hpp)
ROUTES = {"PNG_BATCH": 39, "PNG_BATCH_FILTER": 40, "SUB_BATCHES": 26}
ROUTE_PNG_BATCH, ROUTE_PNG_BATCH_FILTER, ROUTE_SUB_BATCHES = (1 << b for b in ROUTES.values())

NO_RAYON = 1  # flags: semantics of a reference build without the `parallel` feature
EFFORT_HIGH = 2  # flags, read by `encode` / `encode_device`: the device DEFLATE's denser effort (hash chains, lazy parse)


def filtered_size(width, height, bytes_per_pixel):
    return height * (width * bytes_per_pixel + 1)


def apply_filters(data, width, height, bytes_per_pixel, strategy=FilterStrategy.ADAPTIVE, flags=0):
    """Host pixels -> (filtered stream as uint8 array [height * (row_bytes + 1)], adler32)."""
    L = _lib.load()
    px = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    out = np.empty(filtered_size(width, height, bytes_per_pixel), np.uint8)
    ad = C.c_uint32()
    rc = L.pixo_hip_png_filter(px.ctypes.data, px.size, width, height, bytes_per_pixel, int(strategy), flags,
                               out.ctypes.data, out.size, C.byref(ad))
    _lib.check(rc)
    return out, ad.value


def apply_filters_device(d_data, width, height, bytes_per_pixel, d_out, strategy=FilterStrategy.ADAPTIVE, flags=0):
    """Device pixels (torch tensor / raw pointer) -> filtered stream written to d_out; returns adler32."""
    L = _lib.load()

    ad = C.c_uint32()
    rc = L.pixo_hip_png_filter_device(_lib.ptr(d_data), width, height, bytes_per_pixel, int(strategy), flags, _lib.ptr(d_out), C.byref(ad))
    _lib.check(rc)
    return ad.value


def apply_filters_async(d_data, width, height, bytes_per_pixel, d_out, d_row_sums, d_scratch,
                        strategy=FilterStrategy.ADAPTIVE, flags=0, stream=0):
    """Enqueue only (no synchronisation): d_row_sums receives 2 u64 per row; combine a host copy of
    them with `adler32_from_row_sums`."""
    L = _lib.load()

    rc = L.pixo_hip_png_filter_async(_lib.ptr(d_data), width, height, bytes_per_pixel, int(strategy), flags, _lib.ptr(d_out),
                                     _lib.ptr(d_row_sums), _lib.ptr(d_scratch), C.c_void_p(stream) if stream else None)
    _lib.check(rc)


def adler32_from_row_sums(row_sums, width, height, bytes_per_pixel):
    L = _lib.load()
    a = np.ascontiguousarray(row_sums, dtype=np.uint64)
    assert a.size == 2 * height
    return int(L.pixo_hip_png_adler32_from_row_sums(a.ctypes.data, width, height, bytes_per_pixel)) & 0xFFFFFFFF


# ---- the prepared stream: reductions + filters (src/png/mod.rs:513-568) -----------------------------------------------

class QuantizationMode(enum.IntEnum):
    """`pixo::png::QuantizationMode`"""
    OFF = 0
    AUTO = 1
    FORCE = 2


class QuantizationOptions:
    """`pixo::png::QuantizationOptions`: Off, 256 colours, no dithering by default."""

    def __init__(self, mode=QuantizationMode.OFF, max_colors=256, dithering=False):
        self.mode, self.max_colors, self.dithering = QuantizationMode(mode), int(max_colors), bool(dithering)

    def to_c(self):
        return _lib.PngQuantizationC(int(self.mode), self.dithering, self.max_colors)

    def __eq__(self, other):
        return isinstance(other, QuantizationOptions) and (self.mode, self.max_colors, self.dithering) == (other.mode, other.max_colors, other.dithering)

    def __repr__(self):
        return "QuantizationOptions(mode=%s, max_colors=%d, dithering=%s)" % (self.mode.name, self.max_colors, self.dithering)


class PngOptions:
    """The fields of `pixo::png::PngOptions` (src/png/mod.rs:41-100).  `compression_level` selects the zlib header's
    FLEVEL and nothing else, and `optimal_compression` compresses the same way: the device DEFLATE has two efforts, but the
    default one is what every value of the reference's knobs gets, so that existing callers keep their bytes.  The denser
    effort, for smooth content (screenshots, charts, gradients), is `flags=EFFORT_HIGH`.  `quantization` travels
    beside the C struct (pixo_png_quantization): `encode` takes the lossy entries when its mode is not Off."""

    def __init__(self, width=0, height=0, color_type=ColorType.Rgba, compression_level=2,
                 filter_strategy=FilterStrategy.ADAPTIVE_FAST, optimize_alpha=False, reduce_color_type=False,
                 strip_metadata=False, reduce_palette=False, optimal_compression=False, flags=0, quantization=None):
        self.quantization = quantization if quantization is not None else QuantizationOptions()
        self.width, self.height, self.color_type = width, height, ColorType(color_type)
        self.compression_level, self.filter_strategy = compression_level, FilterStrategy(filter_strategy)
        self.optimize_alpha, self.reduce_color_type, self.reduce_palette = bool(optimize_alpha), bool(reduce_color_type), bool(reduce_palette)
        self.strip_metadata, self.optimal_compression, self.flags = bool(strip_metadata), bool(optimal_compression), flags

    @classmethod
    def fast(cls, width, height):
        return cls(width, height)

    @classmethod
    def balanced(cls, width, height):
        return cls(width, height, compression_level=6, filter_strategy=FilterStrategy.ADAPTIVE, optimize_alpha=True,
                   reduce_color_type=True, strip_metadata=True, reduce_palette=True)

    @classmethod
    def max(cls, width, height):
        return cls(width, height, compression_level=9, filter_strategy=FilterStrategy.BIGRAMS, optimize_alpha=True,
                   reduce_color_type=True, strip_metadata=True, reduce_palette=True, optimal_compression=True)

    @classmethod
    def from_preset(cls, width, height, preset):
        return cls.fast(width, height) if preset == 0 else cls.max(width, height) if preset == 2 else cls.balanced(width, height)

    @classmethod
    def from_preset_with_lossless(cls, width, height, preset, lossless):
        """mod.rs:203-213: not lossless = Auto, 256 colours, dithering on"""
        o = cls.from_preset(width, height, preset)
        if not lossless:
            o.quantization = QuantizationOptions(QuantizationMode.AUTO, 256, True)
        return o

    @classmethod
    def builder(cls, width, height):
        return PngOptionsBuilder(width, height)

    def to_c(self):
        return _lib.PngOptionsC(self.width, self.height, int(self.color_type), int(self.filter_strategy), self.optimize_alpha,
                                self.reduce_color_type, self.reduce_palette, self.compression_level, self.optimal_compression,
                                self.strip_metadata, self.flags)

    def full_size(self):
        """Bytes that always hold the prepared stream: the unreduced filtered size."""
        return filtered_size(self.width, self.height, self.color_type.bytes_per_pixel())


class PngOptionsBuilder:
    """`PngOptionsBuilder` (src/png/mod.rs:220-340).  Of the quantisation setters it has `quantization_mode`,
    `quantization_max_colors` and `quantization_dithering` (:297-324)."""

    def __init__(self, width, height):
        self._o = PngOptions(width, height)

    def preset(self, preset):  # keeps dimensions and colour type (mod.rs:327-334)
        keep = self._o
        self._o = PngOptions.from_preset(keep.width, keep.height, preset)
        self._o.color_type, self._o.flags = keep.color_type, keep.flags
        return self

    def quantization_mode(self, mode):
        self._o.quantization.mode = QuantizationMode(mode)
        return self

    def quantization_max_colors(self, max_colors):
        self._o.quantization.max_colors = int(max_colors)
        return self

    def quantization_dithering(self, dithering):
        self._o.quantization.dithering = bool(dithering)
        return self

    def build(self):
        return self._o


def _setter(name, conv):
    def f(self, value):
        setattr(self._o, name, conv(value))
        return self
    f.__name__ = name
    return f


for _name, _conv in (("color_type", ColorType), ("compression_level", int), ("filter_strategy", FilterStrategy),
                     ("optimize_alpha", bool), ("reduce_color_type", bool), ("strip_metadata", bool), ("reduce_palette", bool),
                     ("optimal_compression", bool), ("flags", int)):
    setattr(PngOptionsBuilder, _name, _setter(_name, _conv))


class PngLayout:
    """What goes around the IDAT data of a prepared stream (pixo_png_layout)."""

    def __init__(self, c):
        self.color_type_byte, self.bit_depth, self.bytes_per_pixel = c.color_type_byte, c.bit_depth, c.bytes_per_pixel
        self.row_bytes, self.has_trns = c.row_bytes, bool(c.has_trns)
        self.palette = [tuple(c.palette[i]) for i in range(c.palette_len)]  # RGBA, final order

    def __repr__(self):
        return "PngLayout(color_type_byte=%d, bit_depth=%d, bytes_per_pixel=%d, row_bytes=%d, palette=%d entries, has_trns=%s)" % (
            self.color_type_byte, self.bit_depth, self.bytes_per_pixel, self.row_bytes, len(self.palette), self.has_trns)


def prepare(data, options):
    """Host pixels -> (prepared stream as uint8 array, PngLayout, adler32)."""
    L = _lib.load()
    px = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    out = np.empty(max(options.full_size(), 1), np.uint8)
    o, lay, n, ad = options.to_c(), _lib.PngLayoutC(), C.c_size_t(), C.c_uint32()
    rc = L.pixo_hip_png_prepare(px.ctypes.data, px.size, C.byref(o), out.ctypes.data, out.size, C.byref(n), C.byref(lay), C.byref(ad))
    _lib.check(rc)
    return out[:n.value], PngLayout(lay), ad.value


def prepare_device(d_pixels, options, d_out):
    """Device pixels (torch tensor / raw pointer) -> prepared stream in d_out (capacity options.full_size());
    returns (stream length, PngLayout, adler32)."""
    L = _lib.load()

    o, lay, n, ad = options.to_c(), _lib.PngLayoutC(), C.c_size_t(), C.c_uint32()
    rc = L.pixo_hip_png_prepare_device(_lib.ptr(d_pixels), C.byref(o), _lib.ptr(d_out), C.byref(lay), C.byref(n), C.byref(ad))
    _lib.check(rc)
    return n.value, PngLayout(lay), ad.value


def palette_order(counts, matrix):
    """Histogram + co-occurrence matrix of the sorted-key indices -> final order (host only, no GPU)."""
    L = _lib.load()
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    m = np.ascontiguousarray(matrix, dtype=np.uint32)
    n = cnt.size
    assert m.shape == (n, n)
    order = np.empty(n, np.uint8)
    rc = L.pixo_hip_png_palette_order(cnt.ctypes.data, m.ctypes.data, n, order.ctypes.data)
    _lib.check(rc)
    return order


def _chunk(kind, body):
    import struct
    import zlib
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def ihdr_plte_trns(layout, width, height):
    """The IHDR, PLTE and tRNS chunks the reference writes for this layout (src/png/mod.rs:526-547): what `encode` puts
    in front of its IDAT chunks, for callers that assemble a file around a prepared stream themselves."""
    import struct
    out = _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, layout.bit_depth, layout.color_type_byte, 0, 0, 0))
    if layout.palette:
        out += _chunk(b"PLTE", b"".join(bytes(p[:3]) for p in layout.palette))
        if layout.has_trns:
            out += _chunk(b"tRNS", bytes(p[3] for p in layout.palette))
    return out


# ---- whole files: DEFLATE, CRC-32 and chunk writing on the device -----------------------------------------------------

def stored_bound(n):
    """Bytes that always hold the zlib stream of n bytes."""
    return n + 5 * ((n + 65534) // 65535) + 6


def deflate_effort_params():
    """-> (substep, probes) of the high effort: positions whose look-ups come before their inserts, chain entries tried."""
    s, k = C.c_uint32(), C.c_uint32()
    _lib.load().pixo_hip_png_deflate_effort_params(C.byref(s), C.byref(k))
    return s.value, k.value


def zlib_compress(data, level=6, bpp=0, row=0, effort=0):
    """Host bytes -> zlib stream (bytes), compressed on the device.  level: header bits only; bpp / row: distances the
    match search tries besides 1 and its hash table's (0: none); effort: 0 the default finder, 1 the high effort that
    `EFFORT_HIGH` selects for whole files (anything else raises)."""
    L = _lib.load()
    a = flat_u8(data)
    p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    rc = L.pixo_hip_zlib_compress_effort(a.ctypes.data if a.size else None, a.size, level, bpp, row, effort, C.byref(p), C.byref(n))
    _lib.check(rc)
    return _lib.take(L, p, n)


def zlib_compress_device(d_data, length, d_out, capacity, level=6, bpp=0, row=0, effort=0):
    """Device bytes -> zlib stream in d_out (capacity >= stored_bound(length)); returns the stream's length.  effort: as
    for `zlib_compress`."""
    L = _lib.load()

    n = C.c_size_t()
    rc = L.pixo_hip_zlib_compress_effort_device(_lib.ptr(d_data), length, level, bpp, row, effort, _lib.ptr(d_out), capacity, C.byref(n))
    _lib.check(rc)
    return n.value


def _lossy(options):
    return options.quantization.mode != QuantizationMode.OFF


def encode(data, options):
    """Host pixels -> a finished PNG file (bytes): `pixo::png::encode_with_options`.  With `options.quantization` not Off
    the reference's gate decides between the indexed (lossy) file and this same lossless one."""
    L = _lib.load()
    px = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    o, p, n = options.to_c(), C.POINTER(C.c_uint8)(), C.c_size_t()
    if _lossy(options):
        q = options.quantization.to_c()
        rc = L.pixo_hip_png_encode_lossy(px.ctypes.data, px.size, C.byref(o), C.byref(q), C.byref(p), C.byref(n))
    else:
        rc = L.pixo_hip_png_encode(px.ctypes.data, px.size, C.byref(o), C.byref(p), C.byref(n))
    _lib.check(rc)
    return _lib.take(L, p, n)


def encode_device(d_pixels, options):
    """Device pixels (torch tensor / raw pointer) -> a finished PNG file on the host (bytes)."""
    L = _lib.load()
    o, p, n = options.to_c(), C.POINTER(C.c_uint8)(), C.c_size_t()
    if _lossy(options):
        q = options.quantization.to_c()
        rc = L.pixo_hip_png_encode_lossy_device(_lib.ptr(d_pixels), C.byref(o), C.byref(q), C.byref(p), C.byref(n))
    else:
        rc = L.pixo_hip_png_encode_device(_lib.ptr(d_pixels), C.byref(o), C.byref(p), C.byref(n))
    _lib.check(rc)
    return _lib.take(L, p, n)


# ---- batches: equally sized images, one pass of filters, DEFLATE and CRC ------------------------------------------------

def _quant_arg(options):
    return C.byref(options.quantization.to_c()) if _lossy(options) else None


def _check_batch_pixels(d_pixels, options, batch):
    """(the C entries take no length for device pixels: whatever carries a size is checked here)"""
    if hasattr(d_pixels, "numel"):
        need = batch * options.width * options.height * options.color_type.bytes_per_pixel()
        have = d_pixels.numel() * d_pixels.element_size()
        if have != need:
            raise ValueError("a batch of %d images of %dx%d needs %d bytes of pixels, the tensor holds %d" % (batch, options.width, options.height, need, have))


def encode_batch_device(d_pixels, options, batch):
    """`batch` equally sized images back to back in HBM (torch tensor / raw pointer) -> list of `batch` PNG files (bytes),
    each byte for byte what `encode_device` returns for its image.  `options.quantization`, when not Off, is passed on."""
    L = _lib.load()
    _check_batch_pixels(d_pixels, options, batch)
    files, lens, o = (C.POINTER(C.c_uint8) * batch)(), (C.c_size_t * batch)(), options.to_c()
    _lib.check(L.pixo_hip_png_encode_batch_device(_lib.ptr(d_pixels), C.byref(o), _quant_arg(options), batch, files, lens))
    return _lib.take_files(L, files, lens, batch)


def encode_batch_device_into(arena, d_pixels, options, batch):
    """The `batch` files back to back in `arena` (a torch uint8 CPU tensor, pinned or not, a numpy uint8 array, or None
    for a size query — which does the device work: a PNG's size is known only after compression).  Returns (offsets,
    lens); raises BufferTooSmall (`.needed`, `.offsets`, `.lens`) when the files do not fit."""
    L = _lib.load()
    _check_batch_pixels(d_pixels, options, batch)
    o, q = options.to_c(), _quant_arg(options)
    return _lib.into_arena(lambda ptr, cap, offsets, lens: L.pixo_hip_png_encode_batch_device_into(
        _lib.ptr(d_pixels), C.byref(o), q, batch, ptr, cap, offsets, lens), arena, batch)


def encode_batch(data, options, batch):
    """Host pixels of `batch` equally sized images back to back -> list of `batch` PNG files (bytes)."""
    L = _lib.load()
    px = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    files, lens, o = (C.POINTER(C.c_uint8) * batch)(), (C.c_size_t * batch)(), options.to_c()
    _lib.check(L.pixo_hip_png_encode_batch(px.ctypes.data, px.size, C.byref(o), _quant_arg(options), batch, files, lens))
    return _lib.take_files(L, files, lens, batch)


# ---- images of individual sizes and colour types in one block ------------------------------------------------------------

# these entries' bits of the route record (a dict of its own: ROUTES above is pinned as the batch entries' complete list)
IMAGES_ROUTES = {"PNG_IMAGES": 45, "PNG_IMAGES_FILTER": 46}
ROUTE_PNG_IMAGES, ROUTE_PNG_IMAGES_FILTER = (1 << b for b in IMAGES_ROUTES.values())


def encode_images_device(block, images, options):
    """Images of individual sizes and colour types anywhere in one block in HBM (torch tensor / raw pointer) -> list of PNG
    files (bytes), file i byte for byte what `encode_device` returns for image i with `options` at its width, height and
    colour type (`options`' own are not read).  `images`: a `_lib.PngImageC` array, a list of (width, height, ColorType,
    offset), or the (tensor, ColorType) views of `decode.decode_png_batch_device` — then `block` may be None.
    `options.quantization`, when not Off, is passed on."""
    L = _lib.load()
    arr, n, base = image_records(images)
    block = images_block(block, base)
    check_block("images", block, arr, n)
    files, lens, o = (C.POINTER(C.c_uint8) * max(n, 1))(), (C.c_size_t * max(n, 1))(), options.to_c()
    _lib.check(L.pixo_hip_png_encode_images_device(_lib.ptr(block), arr, n, C.byref(o), _quant_arg(options), files, lens))
    return _lib.take_files(L, files, lens, n)


def encode_images_device_into(arena, block, images, options):
    """The files back to back in `arena` (as `encode_batch_device_into`: a torch uint8 CPU tensor, pinned or not, a numpy
    uint8 array, or None for a size query).  Returns (offsets, lens); raises BufferTooSmall (`.needed`, `.offsets`, `.lens`)
    when the files do not fit."""
    L = _lib.load()
    arr, n, base = image_records(images)
    block = images_block(block, base)
    check_block("images", block, arr, n)
    o, q = options.to_c(), _quant_arg(options)
    return _lib.into_arena(lambda ptr, cap, offsets, lens: L.pixo_hip_png_encode_images_device_into(
        _lib.ptr(block), arr, n, C.byref(o), q, ptr, cap, offsets, lens), arena, n)


def encode_images(block_bytes, images, options):
    """The same for a block in host memory (what `decode.decode_png_batch` works from) -> list of PNG files (bytes)."""
    L = _lib.load()
    arr, n, _ = image_records(images)
    px = flat_u8(block_bytes)
    files, lens, o = (C.POINTER(C.c_uint8) * max(n, 1))(), (C.c_size_t * max(n, 1))(), options.to_c()
    _lib.check(L.pixo_hip_png_encode_images(px.ctypes.data, px.size, arr, n, C.byref(o), _quant_arg(options), files, lens))
    return _lib.take_files(L, files, lens, n)


def encode_images_plan(images, options, alignment=0) -> dict:
    """What the images entries decide for these records, no GPU needed: `sub_first` (sub-batch k is images sub_first[k] ..
    sub_first[k + 1]), `way_in` (True: a shared filter launch; False: prepared by itself), `run_strategy` (what the
    reference's rules make of the strategy for each image) and `filter_launches` (summed over the sub-batches) for a block
    whose address is `alignment` modulo 16."""
    L = _lib.load()
    arr, n, _ = image_records(images)
    sub_first, subs, launches = (C.c_uint32 * (n + 1))(), C.c_uint32(), C.c_uint32()
    way, run, o = (C.c_uint8 * max(n, 1))(), (C.c_uint8 * max(n, 1))(), options.to_c()
    _lib.check(L.pixo_hip_debug_png_encode_images_plan(arr, n, C.byref(o), _quant_arg(options), alignment, sub_first, C.byref(subs), way, run,
                                                       C.byref(launches)))
    return {"sub_first": list(sub_first[:subs.value + 1]), "way_in": [bool(v) for v in way[:n]],
            "run_strategy": [FilterStrategy(v) for v in run[:n]], "filter_launches": launches.value}


# ---- lossy mode: palette quantisation and dithering on the device ------------------------------------------------------

class Quantized:
    """What `quantize` made of an image: `applied` False when the gate declined (then nothing else is set)."""

    def __init__(self, applied, indices=None, palette=None, trns_len=0):
        self.applied, self.indices, self.palette, self.trns_len = applied, indices, palette, trns_len


def _quantized(applied, indices, pal, n, trns):
    if not applied.value:
        return Quantized(False)
    return Quantized(True, indices, [tuple(int(v) for v in pal[i]) for i in range(n.value)], trns.value)


def quantize(data, options):
    """Host pixels -> Quantized (indices as a uint8 array [height * width], RGBA palette, tRNS length): the reference's
    gate and `quantize_image` for `options.quantization`."""
    L = _lib.load()
    px = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    idx, pal = np.empty(max(options.width * options.height, 1), np.uint8), np.zeros((256, 4), np.uint8)
    o, q, n, trns, applied = options.to_c(), options.quantization.to_c(), C.c_uint32(), C.c_uint32(), C.c_uint8()
    rc = L.pixo_hip_png_quantize(px.ctypes.data, px.size, C.byref(o), C.byref(q), idx.ctypes.data, idx.size, pal.ctypes.data,
                                 C.byref(n), C.byref(trns), C.byref(applied))
    _lib.check(rc)
    return _quantized(applied, idx[:options.width * options.height], pal, n, trns)


def quantize_device(d_pixels, options, d_indices):
    """Device pixels (torch tensor / raw pointer) -> indices in d_indices (width * height bytes in HBM); returns Quantized
    with `indices` None."""
    L = _lib.load()
    pal = np.zeros((256, 4), np.uint8)
    o, q, n, trns, applied = options.to_c(), options.quantization.to_c(), C.c_uint32(), C.c_uint32(), C.c_uint8()
    rc = L.pixo_hip_png_quantize_device(_lib.ptr(d_pixels), C.byref(o), C.byref(q), _lib.ptr(d_indices), pal.ctypes.data, C.byref(n),
                                        C.byref(trns), C.byref(applied))
    _lib.check(rc)
    return _quantized(applied, None, pal, n, trns)


def dither_stats():
    """(chained launches, calls served band by band, chained launches that gave up) of the dither in this process (tests, tools)."""
    a, b, g = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _lib.check(_lib.load().pixo_hip_debug_png_dither_stats(C.byref(a), C.byref(b), C.byref(g)))
    return a.value, b.value, g.value


def median_cut(colors, counts, max_colors):
    """Colour keys (r<<24 | g<<16 | b<<8 | a) + counts -> the median-cut palette before k-means, RGBA rows (host only, no GPU)."""
    L = _lib.load()
    k, cnt = np.ascontiguousarray(colors, dtype=np.uint32), np.ascontiguousarray(counts, dtype=np.uint32)
    assert k.size == cnt.size
    pal, n = np.zeros((256, 4), np.uint8), C.c_uint32()
    rc = L.pixo_hip_png_median_cut(k.ctypes.data, cnt.ctypes.data, k.size, max_colors, pal.ctypes.data, C.byref(n))
    _lib.check(rc)
    return pal[:n.value].copy()
