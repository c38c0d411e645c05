// png_encode_api.cpp — the extern "C" zlib and PNG whole-file entry points (lossless and quantised): the prepared stream (png_reduce_api.cpp) is
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

// One run of the device DEFLATE: len > 0 bytes at d_data on the context's device -> their zlib stream.
struct ZlibJob {
    const void *d_data;
    size_t len;
    uint8_t level;                   // the header's FLEVEL only
    uint32_t hint_bpp, hint_row;     // distances the match search tries besides 1 and its hash table's (0: none)
    void *d_dst = nullptr;           // where the stream goes (null: c.z_stream)
    const uint32_t *adler = nullptr; // the checksum when the caller has it already (only the total comes down then)
    bool framed = false;             // as IDAT bodies (z_framed_size) in c.z_stream; their pieces' CRC-32 are then on the way into c.h_zinfo
    uint32_t effort = 0;             // 0: the table's latest occurrence, greedy; 1: hash chains and a lazy parse (PIXO_PNG_EFFORT_HIGH)
};
int zlib_on_device(Context &c, const ZlibJob &j, uint64_t *stream_len)
{
    const uint64_t chunks = pixo_dev::z_chunks(j.len), bound = stored_bound(j.len);
    const size_t info_bytes = chunks * sizeof(pixo_dev::ZChunkInfo), off_bytes = (chunks + 1) * sizeof(unsigned long long);
    const size_t crc_bytes = j.framed ? static_cast<size_t>((bound + pixo_dev::kCrcPiece - 1) / pixo_dev::kCrcPiece) * 4 : 0;
    int rc;
    if ((rc = c.z_tok.reserve(chunks * pixo_dev::kZTokStride * sizeof(uint32_t))) || (rc = c.z_slots.reserve(chunks * pixo_dev::kZSlot)) ||
        (rc = c.z_info.reserve(info_bytes + off_bytes)) || (rc = c.h_zinfo.reserve(std::max(info_bytes + off_bytes, crc_bytes))))
        return rc;
    if (!j.d_dst && (rc = c.z_stream.reserve(pixo_dev::z_framed_size(bound) + 16))) return rc;
    if (j.framed && (rc = c.z_crc.reserve(crc_bytes))) return rc;
    if (j.effort && (rc = c.z_prev.reserve(chunks * pixo_dev::kZPrevStride * sizeof(uint16_t)))) return rc;
    auto *d_info = c.z_info.as<pixo_dev::ZChunkInfo>();
    auto *d_off = reinterpret_cast<unsigned long long *>(c.z_info.as<uint8_t>() + info_bytes);
    HIP_TRY(pixo_dev::launch_deflate_chunks(j.d_data, j.len, j.hint_bpp, j.hint_row, j.effort, c.z_tok.as<uint32_t>(), j.effort ? c.z_prev.as<uint16_t>() : nullptr, c.z_slots.as<uint8_t>(), d_info, d_off,
                                            c.stream));
    // The blocks' total, the last word of z_info, comes down: alone when the checksum is known, behind all the checksum is made from otherwise
    const size_t all = info_bytes + off_bytes, down = j.adler ? sizeof(unsigned long long) : all;
    HIP_TRY(hipMemcpyAsync(c.h_zinfo.p, c.z_info.as<uint8_t>() + all - down, down, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    const unsigned long long blocks = *reinterpret_cast<const unsigned long long *>(c.h_zinfo.as<uint8_t>() + down - sizeof(unsigned long long));
    const uint32_t adler = j.adler ? *j.adler : adler_of_chunks(c.h_zinfo.as<pixo_dev::ZChunkInfo>(), chunks, j.len);
    *stream_len = 2 + blocks + 4;
    if (*stream_len > bound) return fail(PIXO_ERR_COMPRESSION, "Compression error: device DEFLATE exceeded the stored bound");
    uint8_t head[2];
    zlib_header(j.level, head);
    uint8_t *dst = j.d_dst ? static_cast<uint8_t *>(j.d_dst) : c.z_stream.as<uint8_t>();
    HIP_TRY(pixo_dev::launch_deflate_compact(c.z_slots.as<uint8_t>(), d_info, d_off, chunks, head[0] | (uint32_t{head[1]} << 8), adler, dst, j.framed, c.stream));
    if (j.framed) {
        HIP_TRY(pixo_dev::launch_deflate_crc(dst, *stream_len, c.z_crc.as<uint32_t>(), c.stream));
        const size_t pieces = static_cast<size_t>((*stream_len + pixo_dev::kCrcPiece - 1) / pixo_dev::kCrcPiece);
        HIP_TRY(hipMemcpyAsync(c.h_zinfo.p, c.z_crc.p, pieces * 4, hipMemcpyDeviceToHost, c.stream));
    }
    return PIXO_OK;
}

int bad_effort(uint32_t effort) // an argument out of its enumeration, as for the resize algorithm
{
    return fail(PIXO_ERR_INVALID_COLOR_ARG, "Invalid DEFLATE effort: " + std::to_string(effort) + " (expected 0 or 1)");
}

void empty_zlib(uint8_t level, uint8_t out[8]) // deflate.rs: header, an empty fixed block, Adler-32 of nothing
{
    zlib_header(level, out);
    out[2] = 0x03; out[3] = 0x00;
    out[4] = 0; out[5] = 0; out[6] = 0; out[7] = 1;
}

// Everything in front of the first IDAT chunk: signature, IHDR, and for a palette image PLTE and tRNS (mod.rs:513-547).
// strip_metadata: there is no ancillary chunk to strip (tRNS is kept by the reference as well).
// trns_len: how many alphas tRNS holds — all of them on the lossless path, trimmed on the quantised one (mod.rs:1888-1902)
std::vector<uint8_t> png_head(uint32_t width, uint32_t height, const pixo_png_layout &layout, uint32_t trns_len)
{
    std::vector<uint8_t> head{0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    uint8_t ihdr[13] = {0};
    put_be32(ihdr, width);
    put_be32(ihdr + 4, height);
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
        if (layout.has_trns) append_chunk(head, "tRNS", trns, trns_len);
    }
    return head;
}

// The frames around a stream that lies at `idat` as IDAT bodies (pixo_dev::z_framed_size), and IEND behind the last.  Every
// chunk: length, type, [body], the CRC of type + body joined from its 4 KiB pieces' values (x^n mod P).
void frame_idats(uint8_t *idat, uint64_t stream_len, const uint32_t *piece_crc)
{
    const uint32_t type_crc = crc32_bytes(0, reinterpret_cast<const uint8_t *>("IDAT"), 4), shift_piece = crc32_x_pow(8ull * pixo_dev::kCrcPiece);
    const uint32_t pieces_per_idat = pixo_dev::kIdatBytes / pixo_dev::kCrcPiece;
    const uint64_t idats = (stream_len + pixo_dev::kIdatBytes - 1) / pixo_dev::kIdatBytes;
    for (uint64_t k = 0; k < idats; ++k) {
        const uint64_t s0 = k * pixo_dev::kIdatBytes, body = std::min<uint64_t>(pixo_dev::kIdatBytes, stream_len - s0);
        uint8_t *frame = idat + s0 + 12 * k;
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
    std::memcpy(idat + pixo_dev::z_framed_size(stream_len), iend.data(), 12);
}

// A prepared stream of `len` bytes in c.p_out -> the finished file in a block the caller owns: DEFLATE, copy, frame, deliver.
int png_finish(Context &c, const pixo_png_options &o, const pixo_png_layout &layout, uint32_t trns_len, size_t len, uint32_t adler,
               const PngFilterView &view, uint8_t **out, size_t *out_len)
{
    ZlibJob job{c.p_out.p, len, o.compression_level, view.bpp, view.row};
    job.adler = &adler;
    job.framed = true;
    job.effort = (o.flags & PIXO_PNG_EFFORT_HIGH) ? 1 : 0;
    uint64_t stream_len = 0;
    int rc = zlib_on_device(c, job, &stream_len);
    if (rc) return rc;

    const std::vector<uint8_t> head = png_head(o.width, o.height, layout, trns_len);
    const size_t framed = static_cast<size_t>(pixo_dev::z_framed_size(stream_len)), file_len = head.size() + framed + 12;
    if ((rc = c.h_file.reserve(file_len))) return rc;
    uint8_t *file = c.h_file.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(file + head.size(), c.z_stream.p, framed, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream)); // (the pieces' CRC-32 have arrived as well)
    std::memcpy(file, head.data(), head.size());
    frame_idats(file + head.size(), stream_len, c.h_zinfo.as<uint32_t>());
    return deliver(file, file_len, out, out_len);
}

// Pixels on the context's device -> the finished file: prepare, then png_finish.
int png_file(Context &c, const void *d_px, const pixo_png_options &o, uint8_t **out, size_t *out_len)
{
    int rc = c.p_out.reserve(static_cast<size_t>(o.height) * (static_cast<size_t>(o.width) * bytes_per_pixel(o.color_type) + 1));
    if (rc) return rc;
    pixo_png_layout layout;
    size_t len = 0;
    uint32_t adler = 0;
    PngFilterView view;
    if ((rc = png_prepare_on_device(c, d_px, o, c.p_out.p, &layout, &len, &adler, &view))) return rc;
    return png_finish(c, o, layout, layout.palette_len, len, adler, view, out, out_len);
}

// ... with quantisation (mod.rs:469-511): the gate declines -> png_file; otherwise the indices as an 8-bit, one-byte-per-pixel
// image through the same filter, DEFLATE, CRC and chunk path (encode_indexed_into, :1814-1886).
int png_file_lossy(Context &c, const void *d_px, const pixo_png_options &o, const pixo_png_quantization &q, uint8_t **out, size_t *out_len)
{
    bool applied = false;
    pixo_png_layout layout;
    uint32_t trns_len = 0;
    int rc = png_quantize_on_device(c, d_px, o, q, &applied, &layout, &trns_len);
    if (rc) return rc;
    if (!applied) return png_file(c, d_px, o, out, out_len);
    uint8_t strategy = o.filter_strategy; // :1866-1874: palette-aware filtering
    if (strategy == PIXO_PNG_ADAPTIVE || strategy == PIXO_PNG_ADAPTIVE_FAST || strategy == PIXO_PNG_MINSUM || strategy == PIXO_PNG_BIGRAMS) strategy = PIXO_PNG_NONE;
    int run = 0;
    bool seq = false;
    const size_t len = static_cast<size_t>(o.height) * (static_cast<size_t>(o.width) + 1);
    if ((rc = png_plan(o.width, o.height, static_cast<uint64_t>(o.width) * o.height, 1, strategy, o.flags, &run, &seq)) || (rc = c.p_out.reserve(len))) return rc;
    uint32_t adler = 0;
    if ((rc = png_filter_on_device(c, c.q_index.p, o.width, o.height, 1, run, seq, c.p_out.p, &adler))) return rc;
    return png_finish(c, o, layout, trns_len, len, adler, PngFilterView{1, o.width + 1}, out, out_len);
}

} // namespace

extern "C" {

int pixo_hip_zlib_compress(const uint8_t *data, size_t len, uint8_t level, uint32_t hint_bpp, uint32_t hint_row, uint8_t **out, size_t *out_len)
{
    return pixo_hip_zlib_compress_effort(data, len, level, hint_bpp, hint_row, 0, out, out_len);
}

int pixo_hip_zlib_compress_effort(const uint8_t *data, size_t len, uint8_t level, uint32_t hint_bpp, uint32_t hint_row, uint32_t effort, uint8_t **out,
                                  size_t *out_len)
{
    if (effort > 1) return bad_effort(effort);
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    if (len == 0) {
        uint8_t e[8];
        empty_zlib(level, e);
        return deliver(e, 8, out, out_len);
    }
    PIXO_REQUIRE(data);
    PIXO_THREAD_CONTEXT(c);
    int rc = upload(c, c.p_in, data, len);
    if (rc) return rc;
    uint64_t n = 0;
    ZlibJob job{c.p_in.p, len, level, hint_bpp, hint_row};
    job.effort = effort;
    if ((rc = zlib_on_device(c, job, &n)) || (rc = c.h_file.reserve(n))) return rc;
    HIP_TRY(hipMemcpyAsync(c.h_file.p, c.z_stream.p, n, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return deliver(c.h_file.as<uint8_t>(), n, out, out_len);
}

int pixo_hip_zlib_compress_device(const void *d_data, size_t len, uint8_t level, uint32_t hint_bpp, uint32_t hint_row, void *d_out, size_t capacity,
                                  size_t *out_len)
{
    return pixo_hip_zlib_compress_effort_device(d_data, len, level, hint_bpp, hint_row, 0, d_out, capacity, out_len);
}

int pixo_hip_zlib_compress_effort_device(const void *d_data, size_t len, uint8_t level, uint32_t hint_bpp, uint32_t hint_row, uint32_t effort, void *d_out,
                                         size_t capacity, size_t *out_len)
{
    if (effort > 1) return bad_effort(effort);
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
    ZlibJob job{d_data, len, level, hint_bpp, hint_row, d_out};
    job.effort = effort;
    if ((rc = zlib_on_device(*c, job, &n))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out_len = n;
    return PIXO_OK;
}

void pixo_hip_png_deflate_effort_params(uint32_t *substep, uint32_t *probes)
{
    if (substep) *substep = pixo_dev::kZEffortSubstep;
    if (probes) *probes = pixo_dev::kZEffortProbes;
}

int pixo_hip_png_encode(const uint8_t *data, size_t data_len, const pixo_png_options *options, uint8_t **out, size_t *out_len)
{
    int rc = png_check_options(options, true, data_len);
    if (rc) return rc;
    PIXO_REQUIRE(data);
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    PIXO_THREAD_CONTEXT(c);
    if ((rc = upload(c, c.p_in, data, data_len))) return rc;
    return png_file(c, c.p_in.p, *options, out, out_len);
}

int pixo_hip_png_encode_device(const void *d_pixels, const pixo_png_options *options, uint8_t **out, size_t *out_len)
{
    int rc = png_check_options(options);
    if (rc) return rc;
    PIXO_REQUIRE(d_pixels);
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return png_file(*c, d_pixels, *options, out, out_len);
}

int pixo_hip_png_encode_lossy(const uint8_t *data, size_t data_len, const pixo_png_options *options, const pixo_png_quantization *quantization,
                              uint8_t **out, size_t *out_len)
{
    int rc = png_check_options(options, true, data_len);
    if (rc) return rc;
    PIXO_REQUIRE(data);
    if ((rc = png_check_quantization(quantization))) return rc;
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    PIXO_THREAD_CONTEXT(c);
    if ((rc = upload(c, c.p_in, data, data_len))) return rc;
    return png_file_lossy(c, c.p_in.p, *options, *quantization, out, out_len);
}

int pixo_hip_png_encode_lossy_device(const void *d_pixels, const pixo_png_options *options, const pixo_png_quantization *quantization, uint8_t **out,
                                     size_t *out_len)
{
    int rc = png_check_options(options);
    if (rc) return rc;
    PIXO_REQUIRE(d_pixels);
    if ((rc = png_check_quantization(quantization))) return rc;
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return png_file_lossy(*c, d_pixels, *options, *quantization, out, out_len);
}

} // extern "C"
