// png_encode_api.cpp — the extern "C" zlib and PNG whole-file entry points: the prepared stream (png_reduce_api.cpp) is
// compressed where it lies (png_deflate.hip), its blocks are compacted into the bodies of 256 KiB IDAT chunks, the chunks'
// CRC-32 come from the device in 4 KiB pieces, and only the finished file crosses to the host.  The chunks around IDAT are
// the reference's byte for byte (src/png/mod.rs:513-630); the IDAT body is this library's own DEFLATE.
#include "capi_internal.hpp"
#include "png_deflate.hpp"

#include <algorithm>
#include <vector>

using namespace pixo_capi;
using namespace pixo_pngz;

namespace {

void put_be32(uint8_t *p, uint32_t v) { p[0] = static_cast<uint8_t>(v >> 24); p[1] = static_cast<uint8_t>(v >> 16); p[2] = static_cast<uint8_t>(v >> 8); p[3] = static_cast<uint8_t>(v); }

void append_chunk(std::vector<uint8_t> &f, const char type[4], const uint8_t *body, size_t n) // src/png/chunk.rs
{
    const size_t at = f.size();
    f.resize(at + 12 + n);
    put_be32(&f[at], static_cast<uint32_t>(n));
    std::memcpy(&f[at + 4], type, 4);
    if (n) std::memcpy(&f[at + 8], body, n);
    put_be32(&f[at + 8 + n], crc32_bytes(0, &f[at + 4], 4 + n));
}

uint32_t adler_of_chunks(const pixo_dev::ZChunkInfo *info, uint64_t chunks, uint64_t len)
{
    const uint64_t M = 65521;
    uint64_t s1 = 1, s2 = 0;
    for (uint64_t c = 0; c < chunks; ++c) {
        const uint64_t n = std::min<uint64_t>(pixo_dev::kZChunk, len - c * pixo_dev::kZChunk);
        s2 = (s2 + n % M * s1 + info[c].sum_b % M) % M;
        s1 = (s1 + info[c].sum_a % M) % M;
    }
    return static_cast<uint32_t>((s2 << 16) | s1);
}

// len > 0 bytes at d_data on the context's device -> their zlib stream at d_dst (null: c.z_stream).  framed: laid out as
// IDAT bodies (pixo_dev::z_framed_size) in c.z_stream, and the pieces' CRC-32 are on their way into c.h_zinfo when this
// returns (same stream: the caller synchronises).  adler_known: the checksum when the caller has it already.
int zlib_on_device(Context &c, const void *d_data, size_t len, uint8_t level, uint32_t hint_bpp, uint32_t hint_row, const uint32_t *adler_known,
                   uint8_t *d_dst, bool framed, uint64_t *stream_len)
{
    const uint64_t chunks = pixo_dev::z_chunks(len), bound = stored_bound(len);
    const size_t info_bytes = chunks * sizeof(pixo_dev::ZChunkInfo), off_bytes = (chunks + 1) * sizeof(unsigned long long);
    const size_t crc_bytes = framed ? static_cast<size_t>((bound + pixo_dev::kCrcPiece - 1) / pixo_dev::kCrcPiece) * 4 : 0;
    int rc;
    if ((rc = c.z_tok.reserve(chunks * pixo_dev::kZTokStride * sizeof(uint32_t))) || (rc = c.z_slots.reserve(chunks * pixo_dev::kZSlot)) ||
        (rc = c.z_info.reserve(info_bytes + off_bytes)) || (rc = c.h_zinfo.reserve(std::max(info_bytes + off_bytes, crc_bytes))))
        return rc;
    if (!d_dst && (rc = c.z_stream.reserve(pixo_dev::z_framed_size(bound) + 16))) return rc;
    if (framed && (rc = c.z_crc.reserve(crc_bytes))) return rc;
    auto *d_info = c.z_info.as<pixo_dev::ZChunkInfo>();
    auto *d_off = reinterpret_cast<unsigned long long *>(c.z_info.as<uint8_t>() + info_bytes);
    HIP_TRY(pixo_dev::launch_deflate_chunks(d_data, len, hint_bpp, hint_row, c.z_tok.as<uint32_t>(), c.z_slots.as<uint8_t>(), d_info, d_off, c.stream));
    uint32_t adler = 0;
    unsigned long long blocks = 0;
    if (adler_known) { // only the total comes down
        HIP_TRY(hipMemcpyAsync(c.h_zinfo.p, d_off + chunks, sizeof(blocks), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        blocks = *c.h_zinfo.as<unsigned long long>();
        adler = *adler_known;
    } else {
        HIP_TRY(hipMemcpyAsync(c.h_zinfo.p, d_info, info_bytes + off_bytes, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        blocks = reinterpret_cast<const unsigned long long *>(c.h_zinfo.as<uint8_t>() + info_bytes)[chunks];
        adler = adler_of_chunks(c.h_zinfo.as<pixo_dev::ZChunkInfo>(), chunks, len);
    }
    *stream_len = 2 + blocks + 4;
    if (*stream_len > bound) return fail(PIXO_ERR_COMPRESSION, "Compression error: device DEFLATE exceeded the stored bound");
    uint8_t head[2];
    zlib_header(level, head);
    uint8_t *dst = d_dst ? d_dst : c.z_stream.as<uint8_t>();
    HIP_TRY(pixo_dev::launch_deflate_compact(c.z_slots.as<uint8_t>(), d_info, d_off, chunks, head[0] | (uint32_t{head[1]} << 8), adler, dst, framed, c.stream));
    if (framed) {
        HIP_TRY(pixo_dev::launch_deflate_crc(dst, *stream_len, c.z_crc.as<uint32_t>(), c.stream));
        const size_t pieces = static_cast<size_t>((*stream_len + pixo_dev::kCrcPiece - 1) / pixo_dev::kCrcPiece);
        HIP_TRY(hipMemcpyAsync(c.h_zinfo.p, c.z_crc.p, pieces * 4, hipMemcpyDeviceToHost, c.stream));
    }
    return PIXO_OK;
}

void empty_zlib(uint8_t level, uint8_t out[8]) // deflate.rs: header, an empty fixed block, Adler-32 of nothing
{
    zlib_header(level, out);
    out[2] = 0x03; out[3] = 0x00;
    out[4] = 0; out[5] = 0; out[6] = 0; out[7] = 1;
}

// Pixels on the context's device -> the finished file in a block the caller owns.
int png_file(Context &c, const void *d_px, const pixo_png_options &o, uint8_t **out, size_t *out_len)
{
    const uint32_t in_bpp = o.color_type == PIXO_GRAY ? 1u : o.color_type == PIXO_GRAY_ALPHA ? 2u : o.color_type == PIXO_RGB ? 3u : 4u;
    int rc = c.p_out.reserve(static_cast<size_t>(o.height) * (static_cast<size_t>(o.width) * in_bpp + 1));
    if (rc) return rc;
    pixo_png_layout layout;
    size_t len = 0;
    uint32_t adler = 0;
    if ((rc = png_prepare_on_device(c, d_px, o, c.p_out.p, &layout, &len, &adler))) return rc;
    const bool bytewise = layout.bit_depth < 8 || layout.color_type_byte == 3;
    uint64_t stream_len = 0;
    if ((rc = zlib_on_device(c, c.p_out.p, len, o.compression_level, bytewise ? 1u : layout.bytes_per_pixel, layout.row_bytes + 1, &adler, nullptr,
                             true, &stream_len)))
        return rc;

    std::vector<uint8_t> head{0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    uint8_t ihdr[13] = {0};
    put_be32(ihdr, o.width);
    put_be32(ihdr + 4, o.height);
    ihdr[8] = layout.bit_depth;
    ihdr[9] = layout.color_type_byte;
    append_chunk(head, "IHDR", ihdr, 13);
    if (layout.palette_len) {
        uint8_t plte[256 * 3], trns[256];
        for (uint32_t i = 0; i < layout.palette_len; ++i) {
            std::memcpy(plte + 3 * i, layout.palette[i], 3);
            trns[i] = layout.palette[i][3];
        }
        append_chunk(head, "PLTE", plte, 3 * layout.palette_len);
        if (layout.has_trns) append_chunk(head, "tRNS", trns, layout.palette_len);
    }
    const uint64_t idats = (stream_len + pixo_dev::kIdatBytes - 1) / pixo_dev::kIdatBytes;
    const size_t framed = static_cast<size_t>(pixo_dev::z_framed_size(stream_len)), file_len = head.size() + framed + 12;
    if ((rc = c.h_file.reserve(file_len))) return rc;
    uint8_t *file = c.h_file.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(file + head.size(), c.z_stream.p, framed, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream)); // (the pieces' CRC-32 have arrived as well)
    std::memcpy(file, head.data(), head.size());

    // every IDAT chunk: length, type, [body], the CRC of type + body joined from the pieces' values (x^n mod P)
    const uint32_t *piece_crc = c.h_zinfo.as<uint32_t>();
    const uint32_t type_crc = crc32_bytes(0, reinterpret_cast<const uint8_t *>("IDAT"), 4), shift_piece = crc32_x_pow(8ull * pixo_dev::kCrcPiece);
    const uint32_t pieces_per_idat = pixo_dev::kIdatBytes / pixo_dev::kCrcPiece;
    for (uint64_t k = 0; k < idats; ++k) {
        const uint64_t s0 = k * pixo_dev::kIdatBytes, body = std::min<uint64_t>(pixo_dev::kIdatBytes, stream_len - s0);
        uint8_t *frame = file + head.size() + s0 + 12 * k;
        put_be32(frame, static_cast<uint32_t>(body));
        std::memcpy(frame + 4, "IDAT", 4);
        uint32_t crc = type_crc;
        for (uint64_t at = 0, j = k * pieces_per_idat; at < body; at += pixo_dev::kCrcPiece, ++j) {
            const uint64_t n = std::min<uint64_t>(pixo_dev::kCrcPiece, body - at);
            crc = crc32_multiply(n == pixo_dev::kCrcPiece ? shift_piece : crc32_x_pow(8 * n), crc) ^ piece_crc[j];
        }
        put_be32(frame + 8 + body, crc);
    }
    std::vector<uint8_t> iend;
    append_chunk(iend, "IEND", nullptr, 0);
    std::memcpy(file + head.size() + framed, iend.data(), 12);
    // strip_metadata: the file has no ancillary chunk to strip (tRNS is kept by the reference as well)
    return deliver(file, file_len, out, out_len);
}

} // namespace

extern "C" {

int pixo_hip_zlib_compress(const uint8_t *data, size_t len, uint8_t level, uint32_t hint_bpp, uint32_t hint_row, uint8_t **out, size_t *out_len)
{
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    if (len == 0) {
        uint8_t e[8];
        empty_zlib(level, e);
        return deliver(e, 8, out, out_len);
    }
    PIXO_REQUIRE(data);
    Context &c = thread_context();
    int rc = c.ensure();
    if (rc) return rc;
    PIXO_ON_DEVICE_OF(c);
    if ((rc = c.p_in.reserve((len + 15) & ~size_t{15}))) return rc;
    HIP_TRY(hipMemcpyAsync(c.p_in.p, data, len, hipMemcpyHostToDevice, c.stream));
    uint64_t n = 0;
    if ((rc = zlib_on_device(c, c.p_in.p, len, level, hint_bpp, hint_row, nullptr, nullptr, false, &n))) return rc;
    if ((rc = c.h_file.reserve(n))) return rc;
    HIP_TRY(hipMemcpyAsync(c.h_file.p, c.z_stream.p, n, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return deliver(c.h_file.as<uint8_t>(), n, out, out_len);
}

int pixo_hip_zlib_compress_device(const void *d_data, size_t len, uint8_t level, uint32_t hint_bpp, uint32_t hint_row, void *d_out, size_t capacity,
                                  size_t *out_len)
{
    PIXO_REQUIRE(d_out);
    PIXO_REQUIRE(out_len);
    const uint64_t bound = len ? stored_bound(len) : 8; // (no input: the 8 bytes of the empty stream)
    if (capacity < bound) return too_small(bound, out_len);
    Context *c = nullptr;
    int rc = context_on_current_device(&c);
    if (rc) return rc;
    if (len == 0) {
        uint8_t e[8];
        empty_zlib(level, e);
        HIP_TRY(hipMemcpyAsync(d_out, e, 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        *out_len = 8;
        return PIXO_OK;
    }
    PIXO_REQUIRE(d_data);
    uint64_t n = 0;
    if ((rc = zlib_on_device(*c, d_data, len, level, hint_bpp, hint_row, nullptr, static_cast<uint8_t *>(d_out), false, &n))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out_len = n;
    return PIXO_OK;
}

int pixo_hip_png_encode(const uint8_t *data, size_t data_len, const pixo_png_options *options, uint8_t **out, size_t *out_len)
{
    size_t in_bytes = 0;
    int rc = png_check_options(options, &in_bytes);
    if (rc) return rc;
    if (data_len != in_bytes)
        return fail(PIXO_ERR_INVALID_DATA_LENGTH, "Invalid pixel data length: expected " + std::to_string(in_bytes) + " bytes, got " + std::to_string(data_len));
    if (options->filter_strategy > PIXO_PNG_BIGRAMS) return fail(PIXO_ERR_COMPRESSION, "Compression error: unknown PNG filter strategy");
    PIXO_REQUIRE(data);
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    Context &c = thread_context();
    if ((rc = c.ensure())) return rc;
    PIXO_ON_DEVICE_OF(c);
    if ((rc = c.p_in.reserve((in_bytes + 15) & ~size_t{15}))) return rc;
    HIP_TRY(hipMemcpyAsync(c.p_in.p, data, in_bytes, hipMemcpyHostToDevice, c.stream));
    return png_file(c, c.p_in.p, *options, out, out_len);
}

int pixo_hip_png_encode_device(const void *d_pixels, const pixo_png_options *options, uint8_t **out, size_t *out_len)
{
    size_t in_bytes = 0;
    int rc = png_check_options(options, &in_bytes);
    if (rc) return rc;
    if (options->filter_strategy > PIXO_PNG_BIGRAMS) return fail(PIXO_ERR_COMPRESSION, "Compression error: unknown PNG filter strategy");
    PIXO_REQUIRE(d_pixels);
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return png_file(*c, d_pixels, *options, out, out_len);
}

} // extern "C"
