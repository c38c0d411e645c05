"""A plain sequential restatement of the reference's PNG decoder (src/decode/png.rs:101-626, with the zlib framing of
src/decode/inflate.rs:294-352) in Python.  Test harness only.

It is a restatement, not a run of the reference: the reference's wasm build exports no decoder and there is no Rust toolchain
to build one, so — like the restart-interval branch of the JPEG encoder — this path rests on the restatement and on
independent decoders (tests/test_png_decode_model.py pins it against Pillow and against the raw stream) only.  On a
well-formed file its output is fixed by the PNG and zlib specifications.

The DEFLATE body is inflated by Python's zlib (raw, between the two header bytes and the last four bytes, as the reference
slices it), so the error strings of the block decoders are not the model's: tests state those literally."""
import struct
import zlib

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_DIMENSION = 1 << 24
GRAY, RGB, INDEXED, GRAY_ALPHA, RGBA = 0, 2, 3, 4, 6
NAMES = {GRAY: "Grayscale", RGB: "Rgb", INDEXED: "Indexed", GRAY_ALPHA: "GrayscaleAlpha", RGBA: "Rgba"}
VALID_DEPTHS = {GRAY: (1, 2, 4, 8, 16), RGB: (8, 16), INDEXED: (1, 2, 4, 8), GRAY_ALPHA: (8, 16), RGBA: (8, 16)}
CHANNELS = {GRAY: 1, RGB: 3, INDEXED: 1, GRAY_ALPHA: 2, RGBA: 4}
# pixo::ColorType of the output, and the library's status codes (include/pixo_hip.h)
OUT_GRAY, OUT_GRAY_ALPHA, OUT_RGB, OUT_RGBA = 0, 1, 2, 3
INVALID_DIMENSIONS, IMAGE_TOO_LARGE, INVALID_DECODE, UNSUPPORTED_DECODE = -1, -4, -10, -11


class DecodeError(Exception):
    """status: the C ABI's code; str(e): the reference's Display string"""

    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


def invalid(msg):
    return DecodeError(INVALID_DECODE, "Decode error: " + msg)


def unsupported(msg):
    return DecodeError(UNSUPPORTED_DECODE, "Unsupported: " + msg)


def filter_unit(color_type, depth):
    if color_type == INDEXED:
        return 1
    if color_type == GRAY:
        return max((depth + 7) // 8, 1)
    return CHANNELS[color_type] * depth // 8


def row_bytes(color_type, depth, width):
    if color_type in (GRAY, INDEXED):
        return (width * depth + 7) // 8
    return width * CHANNELS[color_type] * depth // 8


def has_alpha_in_trns(trns):
    return trns is not None and any(v != 255 for v in trns)


def walk(data):
    """png.rs:102-260 -> dict(width, height, depth, color_type, plte, trns, idat, out_color_type)"""
    if len(data) < 8 or data[:8] != SIGNATURE:
        raise invalid("not a PNG file")
    pos, ihdr, idat, plte, trns, seen_iend = 8, None, bytearray(), None, None, False
    while pos + 12 <= len(data):
        length = struct.unpack(">I", data[pos:pos + 4])[0]
        ctype = data[pos + 4:pos + 8]
        end = pos + 8 + length
        if end + 4 > len(data):
            raise invalid("truncated PNG chunk")
        body = data[pos + 8:end]
        if struct.unpack(">I", data[end:end + 4])[0] != zlib.crc32(ctype + body):
            raise invalid("CRC mismatch in %s chunk" % ctype.decode("utf-8", "replace"))
        if ctype == b"IHDR":
            if length != 13:
                raise invalid("invalid IHDR length")
            w, h, depth, ct, comp, flt, lace = struct.unpack(">IIBBBBB", body)
            if ct not in NAMES:
                raise invalid("invalid PNG color type: %d" % ct)
            ihdr = dict(width=w, height=h, depth=depth, color_type=ct, compression=comp, filter=flt, interlace=lace)
        elif ctype == b"PLTE":
            if length % 3:
                raise invalid("invalid PLTE length")
            plte = bytes(body)
        elif ctype == b"tRNS":
            trns = bytes(body)
        elif ctype == b"IDAT":
            idat += body
        elif ctype == b"IEND":
            seen_iend = True
            break
        pos = end + 4
    if not seen_iend:
        raise invalid("missing IEND chunk")
    if ihdr is None:
        raise invalid("missing IHDR chunk")
    w, h = ihdr["width"], ihdr["height"]
    if w == 0 or h == 0:
        raise DecodeError(INVALID_DIMENSIONS, "Invalid image dimensions: %dx%d" % (w, h))
    if w > MAX_DIMENSION or h > MAX_DIMENSION:
        raise DecodeError(IMAGE_TOO_LARGE, "Image %dx%d exceeds maximum dimension %d" % (w, h, MAX_DIMENSION))
    if ihdr["compression"] != 0:
        raise invalid("unsupported compression method")
    if ihdr["filter"] != 0:
        raise invalid("unsupported filter method")
    if ihdr["interlace"] != 0:
        raise unsupported("Adam7 interlaced images not supported")
    ct, depth = ihdr["color_type"], ihdr["depth"]
    if depth not in VALID_DEPTHS[ct]:
        raise invalid("invalid bit depth %d for color type %s" % (depth, NAMES[ct]))
    if not idat:
        raise invalid("no IDAT data")
    out = {GRAY: OUT_GRAY, GRAY_ALPHA: OUT_GRAY_ALPHA, RGBA: OUT_RGBA, RGB: OUT_RGB}.get(ct)
    if ct == INDEXED:
        out = OUT_RGBA if has_alpha_in_trns(trns) else OUT_RGB
    return dict(ihdr, plte=plte, trns=trns, idat=bytes(idat), out_color_type=out)


def info(data):
    f = walk(data)
    return f["width"], f["height"], f["out_color_type"]


def inflate_zlib(data, expected):
    """inflate.rs:294-352 with Some(expected): header checks, the body (Python's zlib), Adler-32 from the last four bytes, size"""
    if len(data) < 6:
        raise invalid("zlib stream too short")
    cmf, flg = data[0], data[1]
    if cmf & 0x0F != 8:
        raise invalid("invalid zlib compression method")
    if ((cmf << 8) | flg) % 31:
        raise invalid("invalid zlib header checksum")
    if flg & 0x20:
        raise unsupported("preset dictionary not supported")
    out = zlib.decompressobj(-15).decompress(data[2:-4])  # (an ill-formed body: zlib.error — the model has no words for it)
    stored, computed = struct.unpack(">I", data[-4:])[0], zlib.adler32(out)
    if stored != computed:
        raise invalid("Adler32 mismatch: expected %08X, got %08X" % (stored, computed))
    if len(out) != expected:
        raise invalid("decompressed size mismatch: expected %d, got %d" % (expected, len(out)))
    return out


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def unfilter_row(ft, row, prev, bpp):
    """png.rs:370-410, in place on a bytearray"""
    n = len(row)
    if ft == 0:
        return
    if ft == 1:
        for i in range(bpp, n):
            row[i] = (row[i] + row[i - bpp]) & 255
    elif ft == 2:
        for i in range(n):
            row[i] = (row[i] + prev[i]) & 255
    elif ft == 3:
        for i in range(n):
            left = row[i - bpp] if i >= bpp else 0
            row[i] = (row[i] + ((left + prev[i]) >> 1)) & 255
    elif ft == 4:
        for i in range(n):
            a = row[i - bpp] if i >= bpp else 0
            c = prev[i - bpp] if i >= bpp else 0
            row[i] = (row[i] + paeth(a, prev[i], c)) & 255
    else:
        raise invalid("invalid filter type: %d" % ft)


def reconstruct(stream, height, rb, bpp):
    """png.rs:343-363 -> the raw rows, concatenated"""
    prev, rows = bytearray(rb), bytearray()
    for y in range(height):
        at = y * (rb + 1)
        row = bytearray(stream[at + 1:at + 1 + rb])
        unfilter_row(stream[at], row, prev, bpp)
        rows += row
        prev = row
    return bytes(rows)


def unpack_row(packed, width, depth):
    """png.rs:567-609"""
    if depth == 8:
        return list(packed[:width])
    per, mask = 8 // depth, (1 << depth) - 1
    return [(packed[x // per] >> ((per - 1 - x % per) * depth)) & mask for x in range(width)]


def scale_to_8bit(s, depth):
    if depth == 1:
        return 255 if s else 0
    if depth == 2:
        return (s | (s << 2) | (s << 4) | (s << 6)) & 255
    if depth == 4:
        return (s | (s << 4)) & 255
    return s


def convert(f, raw):
    """png.rs:430-533"""
    w, h, depth, ct = f["width"], f["height"], f["depth"], f["color_type"]
    rb = row_bytes(ct, depth, w)
    if ct != INDEXED:
        if depth == 8:
            return raw
        if depth == 16:
            return raw[0::2]
        out = bytearray()
        for y in range(h):
            out += bytes(scale_to_8bit(s, depth) for s in unpack_row(raw[y * rb:(y + 1) * rb], w, depth))
        return bytes(out)
    if f["plte"] is None:
        raise invalid("missing PLTE chunk")
    plte, trns = f["plte"], f["trns"]
    entries, rgba = len(plte) // 3, has_alpha_in_trns(f["trns"])
    out = bytearray()
    for y in range(h):
        for idx in unpack_row(raw[y * rb:(y + 1) * rb], w, depth):
            if idx < entries:
                out += plte[3 * idx:3 * idx + 3]
                if rgba:
                    out.append(trns[idx] if idx < len(trns) else 255)
            else:
                out += b"\0\0\0\xff" if rgba else b"\0\0\0"
    return bytes(out)


def decode_png(data):
    """-> (width, height, pixels, pixo ColorType value); raises DecodeError in the reference's order"""
    f = walk(data)
    w, h, depth, ct = f["width"], f["height"], f["depth"], f["color_type"]
    rb = row_bytes(ct, depth, w)
    stream = inflate_zlib(f["idat"], h * (rb + 1))
    raw = reconstruct(stream, h, rb, filter_unit(ct, depth))
    return w, h, convert(f, raw), f["out_color_type"]
