// png_encode_api.cpp — the extern "C" zlib and PNG whole-file entry points (lossless and quantised): the prepared stream (png_reduce_api.cpp) is
// compressed where it lies (png_deflate.hip), its blocks are compacted into the bodies of 256 KiB IDAT chunks, the chunks'
// CRC-32 come from the device in 4 KiB pieces, and only the finished file crosses to the host.  The chunks around IDAT are
// the reference's byte for byte (src/png/mod.rs:513-630); the IDAT body is this library's own DEFLATE.
// There is one tail (tail_begin, tail_finish, tail_deliver) over a table of segments (png_deflate_math.h ZSegment): a single
// file and a bare zlib stream are a table of one, the batch entries run N equal images through it at once, the images
// entries N images of individual sizes and colour types.
// The steps every batch driver takes, and their order: DESIGN.md §4.0; the shared ones: batch_steps.hpp.
#include "batch_steps.hpp"
#include "png_deflate.hpp"
#include "png_filter.hpp"

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

// ---- the tail: prepared streams (segments) -> their zlib streams in one pass of DEFLATE, scan, compaction and CRC ----------
// Every entry ends here: a single file or a bare zlib stream is a table of one segment, a batch one of N.
// One prepared stream, and what its file needs around the IDAT chunks.
struct PngSegment {
    size_t src = 0, len = 0; // its first byte counted from the tail's d_data, its bytes
    PngFilterView view{1, 0}; // distances the match search tries besides 1 and its hash table's (0: none)
    uint32_t adler = 0;
    pixo_png_layout layout;
    uint32_t trns_len = 0;
    uint32_t width = 0, height = 0; // the image's, for its IHDR
};
// Where the files go: blocks the caller owns (files), or back to back into an arena in host memory (offsets).
struct BatchSink {
    uint8_t **files = nullptr;
    bool staged = false; // blocks: none from the pinned pool, every file through the context's pinned file buffer into a fresh malloc block (the single entries)
    uint8_t *arena = nullptr;
    size_t cap = 0;
    size_t *offsets = nullptr, *lens = nullptr;
    bool pinned = false; // the arena is host memory the runtime knows: device-to-host copies go straight into it
    size_t at = 0;       // arena: the bytes of the files so far
    uint32_t waits = 0;  // how often the host has waited for the stream (debug switch trace)
};
int wait_for(Context &c, BatchSink &sink)
{
    ++sink.waits;
    HIP_TRY(hipStreamSynchronize(c.stream));
    return PIXO_OK;
}
uint32_t png_effort(const pixo_png_options &o) { return (o.flags & PIXO_PNG_EFFORT_HIGH) ? 1 : 0; }

// One run of the tail: the segment table, the scratch, the launches.  Host side, in c.h_zinfo: the table, then what comes
// down — the segments' totals and the pieces' CRC-32 of framed streams, the chunks' records of a bare one.
struct BatchTail {
    const void *d_data = nullptr; // what the segments' src count from (set by the caller)
    void *d_dst = nullptr;        // where the streams go (null: c.z_stream)
    bool framed = true;           // as IDAT bodies (z_framed_size) with their pieces' CRC-32; false: the bare zlib stream of one segment, at any address
    uint32_t nseg = 0, chunks = 0, pieces = 0, header = 0;
    size_t table_bytes = 0, info_bytes = 0, totals_bytes = 0;
    ZSegment *h_table = nullptr;
    ZSegment *d_table = nullptr;
    unsigned long long *d_off = nullptr, *d_totals = nullptr; // (the totals in front of the CRC values in c.z_crc: one copy brings both)
    uint8_t *h_down = nullptr;
    const unsigned long long *h_totals() const { return reinterpret_cast<const unsigned long long *>(h_down); }
    const uint32_t *h_crc() const { return reinterpret_cast<const uint32_t *>(h_down + totals_bytes); }
};
// Reserves everything, uploads the table and launches the DEFLATE of every chunk of every segment.  The Adler-32 of the
// segments need not be known yet: the compaction reads them (tail_finish).  level: the header's FLEVEL only; effort 0: the
// table's latest occurrence, greedy; 1: hash chains and a lazy parse (PIXO_PNG_EFFORT_HIGH).
int tail_begin(Context &c, const std::vector<PngSegment> &segs, uint8_t level, uint32_t effort, BatchTail &t)
{
    t.nseg = static_cast<uint32_t>(segs.size());
    std::vector<ZSegment> table(t.nseg + 1);
    for (uint32_t i = 0; i < t.nseg; ++i) table[i] = ZSegment{segs[i].src, segs[i].len, 0, 0, 0, segs[i].view.bpp, segs[i].view.row, segs[i].adler, 0};
    if (!seg_layout(table.data(), t.nseg)) return hip_fail(hipErrorInvalidValue, "chunks of a PNG batch");
    t.chunks = table[t.nseg].first_chunk;
    t.pieces = table[t.nseg].first_piece;
    t.table_bytes = table.size() * sizeof(ZSegment);
    t.info_bytes = t.chunks * sizeof(pixo_dev::ZChunkInfo);
    t.totals_bytes = t.nseg * sizeof(unsigned long long);
    const size_t off_bytes = t.chunks * sizeof(unsigned long long), crc_bytes = t.framed ? static_cast<size_t>(t.pieces) * 4 : 0;
    int rc;
    if ((rc = c.z_tok.reserve(static_cast<size_t>(t.chunks) * pixo_dev::kZTokStride * sizeof(uint32_t))) ||
        (rc = c.z_slots.reserve(static_cast<size_t>(t.chunks) * pixo_dev::kZSlot)) || (rc = c.z_info.reserve(t.info_bytes + off_bytes + t.table_bytes)) ||
        (rc = c.h_zinfo.reserve(t.table_bytes + std::max(t.totals_bytes + crc_bytes, t.info_bytes))) || (rc = c.z_crc.reserve(t.totals_bytes + crc_bytes)))
        return rc;
    if (!t.d_dst && (rc = c.z_stream.reserve(static_cast<size_t>(table[t.nseg].dst) + 16))) return rc;
    if (effort && (rc = c.z_prev.reserve(static_cast<size_t>(t.chunks) * pixo_dev::kZPrevStride * sizeof(uint16_t)))) return rc;
    uint8_t *d = c.z_info.as<uint8_t>(), *h = c.h_zinfo.as<uint8_t>();
    t.d_off = reinterpret_cast<unsigned long long *>(d + t.info_bytes);
    t.d_table = reinterpret_cast<ZSegment *>(d + t.info_bytes + off_bytes);
    t.d_totals = c.z_crc.as<unsigned long long>();
    t.h_table = reinterpret_cast<ZSegment *>(h);
    t.h_down = h + t.table_bytes;
    std::memcpy(t.h_table, table.data(), t.table_bytes);
    uint8_t head[2];
    zlib_header(level, head);
    t.header = head[0] | (uint32_t{head[1]} << 8);
    HIP_TRY(hipMemcpyAsync(t.d_table, t.h_table, t.table_bytes, hipMemcpyHostToDevice, c.stream));
    HIP_TRY(pixo_dev::launch_deflate(t.d_data, t.d_table, t.nseg, t.chunks, effort, c.z_tok.as<uint32_t>(), effort ? c.z_prev.as<uint16_t>() : nullptr,
                                     c.z_slots.as<uint8_t>(), c.z_info.as<pixo_dev::ZChunkInfo>(), c.stream));
    return PIXO_OK;
}
// Scan, compaction and CRC over all segments; the totals and piece values of framed streams are on their way down behind
// them.  adlers_late: the segments' checksums became known after tail_begin (the stream has been synchronised since): the
// table goes up once more.
int tail_finish(Context &c, const std::vector<PngSegment> &segs, BatchTail &t, bool adlers_late)
{
    if (adlers_late) {
        for (uint32_t i = 0; i < t.nseg; ++i) t.h_table[i].adler = segs[i].adler;
        HIP_TRY(hipMemcpyAsync(t.d_table, t.h_table, t.table_bytes, hipMemcpyHostToDevice, c.stream));
    }
    uint32_t *d_crc = t.framed ? reinterpret_cast<uint32_t *>(c.z_crc.as<uint8_t>() + t.totals_bytes) : nullptr;
    HIP_TRY(pixo_dev::launch_deflate_finish(c.z_slots.as<uint8_t>(), c.z_info.as<pixo_dev::ZChunkInfo>(), t.d_table, t.nseg, t.chunks, t.pieces, t.header, t.d_off,
                                            t.d_totals, t.d_dst ? static_cast<uint8_t *>(t.d_dst) : c.z_stream.as<uint8_t>(), t.framed, d_crc, c.stream));
    if (t.framed) HIP_TRY(hipMemcpyAsync(t.h_down, c.z_crc.p, t.totals_bytes + static_cast<size_t>(t.pieces) * 4, hipMemcpyDeviceToHost, c.stream));
    return PIXO_OK;
}
// Copy, frame, deliver: the framed streams behind their heads, in the caller's blocks or at their arena offsets; frames and
// IEND by the host.  first: the segments' first image in the sink.
int tail_deliver(Context &c, const std::vector<PngSegment> &segs, const BatchTail &t, uint32_t first, BatchSink &sink)
{
    struct File { std::vector<uint8_t> head; uint64_t stream_len = 0; size_t framed = 0, len = 0; uint8_t *at = nullptr; bool staged = false; };
    std::vector<File> f(t.nseg);
    for (uint32_t i = 0; i < t.nseg; ++i) {
        f[i].stream_len = 2 + t.h_totals()[i] + 4;
        if (f[i].stream_len > stored_bound(segs[i].len)) return fail(PIXO_ERR_COMPRESSION, "Compression error: device DEFLATE exceeded the stored bound");
        f[i].head = png_head(segs[i].width, segs[i].height, segs[i].layout, segs[i].trns_len);
        f[i].framed = static_cast<size_t>(pixo_dev::z_framed_size(f[i].stream_len));
        f[i].len = f[i].head.size() + f[i].framed + 12;
        sink.lens[first + i] = f[i].len;
    }
    // Blocks: from the pinned pool, the copies go straight into them.  Arena: straight into a pinned one.  Otherwise (the sink
    // asks for it, the pool is exhausted, the arena is pageable) through the context's pinned file buffer.
    size_t stage = 0;
    if (sink.files) {
        bool pooled = !sink.staged;
        for (uint32_t i = 0; i < t.nseg && pooled; ++i)
            if (!(sink.files[first + i] = pool_take(f[i].len))) pooled = false;
        for (uint32_t i = 0; i < t.nseg; ++i) {
            if (pooled) { f[i].at = sink.files[first + i]; continue; }
            free_file(sink.files[first + i]);
            sink.files[first + i] = nullptr;
            f[i].staged = true;
            stage += f[i].len;
        }
    } else {
        for (uint32_t i = 0; i < t.nseg; ++i) {
            sink.offsets[first + i] = sink.at;
            sink.at += f[i].len;
        }
        // (nothing is copied from the sub-batch on that no longer fits: sizes only from there on)
        for (uint32_t i = 0; i < t.nseg && sink.arena && sink.at <= sink.cap; ++i) {
            if (sink.pinned) f[i].at = sink.arena + sink.offsets[first + i];
            else { f[i].staged = true; stage += f[i].len; }
        }
    }
    if (stage) {
        if (const int rc = c.h_file.reserve(stage)) return rc;
        size_t at = 0;
        for (File &x : f)
            if (x.staged) { x.at = c.h_file.as<uint8_t>() + at; at += x.len; }
    }
    hipError_t e = hipSuccess;
    bool any = false;
    for (uint32_t i = 0; i < t.nseg && e == hipSuccess; ++i)
        if (f[i].at) { any = true; e = hipMemcpyAsync(f[i].at + f[i].head.size(), c.z_stream.as<uint8_t>() + t.h_table[i].dst, f[i].framed, hipMemcpyDeviceToHost, c.stream); }
    for (const File &x : f)
        if (x.at) std::memcpy(x.at, x.head.data(), x.head.size()); // (while the copies run: they touch other bytes)
    if (any) { // (also after an error: no copy is in flight when a block goes back)
        ++sink.waits;
        const hipError_t idle = hipStreamSynchronize(c.stream);
        if (e == hipSuccess) e = idle;
    }
    if (e != hipSuccess) return hip_fail(e, "device-to-host copy of the PNG files");
    for (uint32_t i = 0; i < t.nseg; ++i) {
        if (!f[i].at) continue;
        frame_idats(f[i].at + f[i].head.size(), f[i].stream_len, t.h_crc() + t.h_table[i].first_piece);
        if (!f[i].staged) continue;
        if (sink.files) {
            size_t n = 0;
            if (const int rc = deliver(f[i].at, f[i].len, &sink.files[first + i], &n)) return rc;
        } else {
            std::memcpy(sink.arena + sink.offsets[first + i], f[i].at, f[i].len);
        }
    }
    return PIXO_OK;
}

// One image's prepared stream at c.p_out + seg.src: reduced and filtered, or with q (mod.rs:469-511) and where its gate
// applies the indices as an 8-bit, one-byte-per-pixel image through the same filters (encode_indexed_into, :1814-1886).
// c.p_out is reserved here for a stream that ends where this one does: a batch has reserved all its images' before the
// first, so nothing moves under the streams in front.
int png_segment_of_image(Context &c, const void *d_img, const pixo_png_options &o, const pixo_png_quantization *q, PngSegment &seg)
{
    int rc;
    if (q) {
        bool applied = false;
        if ((rc = png_quantize_on_device(c, d_img, o, *q, &applied, &seg.layout, &seg.trns_len))) return rc;
        if (applied) {
            uint8_t strategy = o.filter_strategy; // :1866-1874: palette-aware filtering
            if (strategy == PIXO_PNG_ADAPTIVE || strategy == PIXO_PNG_ADAPTIVE_FAST || strategy == PIXO_PNG_MINSUM || strategy == PIXO_PNG_BIGRAMS) strategy = PIXO_PNG_NONE;
            int run = 0;
            bool seq = false;
            seg.len = static_cast<size_t>(o.height) * (static_cast<size_t>(o.width) + 1);
            seg.view = PngFilterView{1, o.width + 1};
            if ((rc = png_plan(o.width, o.height, static_cast<uint64_t>(o.width) * o.height, 1, strategy, o.flags, &run, &seq)) || (rc = c.p_out.reserve(seg.src + seg.len)))
                return rc;
            return png_filter_on_device(c, c.q_index.p, o.width, o.height, 1, run, seq, c.p_out.as<uint8_t>() + seg.src, &seg.adler);
        }
    }
    if ((rc = c.p_out.reserve(seg.src + static_cast<size_t>(o.height) * (static_cast<size_t>(o.width) * bytes_per_pixel(o.color_type) + 1)))) return rc;
    if ((rc = png_prepare_on_device(c, d_img, o, c.p_out.as<uint8_t>() + seg.src, &seg.layout, &seg.len, &seg.adler, &seg.view))) return rc;
    seg.trns_len = seg.layout.palette_len;
    return PIXO_OK;
}

// Pixels on the context's device -> the finished file in a block the caller owns: one segment through the tail, delivered
// through the context's pinned file buffer.  The host waits twice behind the prepare stage's own: for the total, for the file.
int png_file(Context &c, const void *d_px, const pixo_png_options &o, const pixo_png_quantization *q, uint8_t **out, size_t *out_len)
{
    std::vector<PngSegment> seg(1);
    seg[0].width = o.width;
    seg[0].height = o.height;
    int rc = png_segment_of_image(c, d_px, o, q, seg[0]);
    if (rc) return rc;
    uint8_t *file = nullptr;
    size_t file_len = 0;
    BatchSink sink;
    sink.files = &file;
    sink.lens = &file_len;
    sink.staged = true;
    BatchTail tail;
    tail.d_data = c.p_out.p;
    if ((rc = tail_begin(c, seg, o.compression_level, png_effort(o), tail)) || (rc = tail_finish(c, seg, tail, false)) || (rc = wait_for(c, sink)) ||
        (rc = tail_deliver(c, seg, tail, 0, sink)))
        return rc;
    if (debug().trace) std::fprintf(stderr, "[pixo_hip] png file: %u chunk(s), host waits %u (behind the image's own)\n", tail.chunks, sink.waits);
    *out = file;
    *out_len = file_len;
    return PIXO_OK;
}

// len > 0 bytes at d_data on the context's device -> their bare zlib stream at d_dst (null: c.z_stream): one unframed segment
// through the tail.  The checksum is not known up front: the chunks' records come down behind the DEFLATE, the host joins
// their sums (and adds up the blocks' bytes: the stream's length), and the table goes up again with it.  One wait here;
// the launches of tail_finish are in flight on return.
int zlib_stream(Context &c, const void *d_data, size_t len, uint8_t level, uint32_t hint_bpp, uint32_t hint_row, uint32_t effort, void *d_dst,
                BatchSink &sink, uint64_t *stream_len)
{
    std::vector<PngSegment> seg(1);
    seg[0].len = len;
    seg[0].view = PngFilterView{hint_bpp, hint_row};
    BatchTail tail;
    tail.d_data = d_data;
    tail.d_dst = d_dst;
    tail.framed = false;
    int rc = tail_begin(c, seg, level, effort, tail);
    if (rc) return rc;
    const auto *info = reinterpret_cast<const pixo_dev::ZChunkInfo *>(tail.h_down);
    HIP_TRY(hipMemcpyAsync(tail.h_down, c.z_info.p, tail.info_bytes, hipMemcpyDeviceToHost, c.stream));
    if ((rc = wait_for(c, sink))) return rc;
    seg[0].adler = adler_of_chunks(info, tail.chunks, len);
    uint64_t blocks = 0;
    for (uint32_t k = 0; k < tail.chunks; ++k) blocks += info[k].bytes;
    *stream_len = 2 + blocks + 4;
    if (*stream_len > stored_bound(len)) return fail(PIXO_ERR_COMPRESSION, "Compression error: device DEFLATE exceeded the stored bound");
    return tail_finish(c, seg, tail, true);
}

// ---- batches: N equal images, one pass of filters, DEFLATE and CRC ("segments") ------------------------
// `batch` images back to back at d_px -> their files into the sink.  Sub-batches run one after the other on the context.  A
// sub-batch holds at most 64 MiB of prepared stream AND at most kBatchChunks chunks, and always at least one image: the
// scratch is per CHUNK, not per byte — kZTokStride * 4 + kZSlot = 327,696 bytes for every chunk however short (524,304 with
// the high effort's links) — and every image has at least one.  1024 chunks: 336 MB of scratch, 537 MB with the high effort,
// what 64 MiB of stream in full chunks need; a batch of thumbnails reaches the chunk limit long before the byte limit.
constexpr uint64_t kBatchChunks = 1024;
int png_batch(Context &c, const void *d_px, const pixo_png_options &o, const pixo_png_quantization *q, uint32_t batch, BatchSink &sink)
{
    const uint32_t bpp = bytes_per_pixel(o.color_type);
    const size_t px_bytes = static_cast<size_t>(o.width) * o.height * bpp, full = static_cast<size_t>(o.height) * (static_cast<size_t>(o.width) * bpp + 1);
    int run = 0;
    bool seq = false;
    int rc = png_plan(o.width, o.height, static_cast<uint64_t>(o.width) * o.height, bpp, o.filter_strategy, o.flags, &run, &seq);
    if (rc) return rc;
    // The batched way in: the stream is the unreduced rows' and the filters do not depend on row 0's decision.  Everything
    // else prepares image by image (the reductions' and the quantiser's own round trips stay) in front of the batched tail.
    const bool filter_batch = !q && !o.optimize_alpha && !o.reduce_color_type && !o.reduce_palette && !seq;
    const uint64_t limit = debug().png_batch_bytes ? debug().png_batch_bytes : (uint64_t{64} << 20);
    const uint64_t by_bytes = std::max<uint64_t>(limit / full, 1), by_chunks = std::max<uint64_t>(kBatchChunks / seg_chunks(full), 1);
    const uint32_t per = static_cast<uint32_t>(std::min<uint64_t>(std::min(by_bytes, by_chunks), batch)); // (a reduced stream is never longer than `full`)
    note_route(route::PNG_BATCH | (filter_batch ? route::PNG_BATCH_FILTER : 0) | (per < batch ? route::SUB_BATCHES : 0));
    for (uint32_t first = 0, part = 0; first < batch; first += per, ++part) {
        const uint32_t nb = std::min(per, batch - first), waits0 = sink.waits;
        const uint8_t *d_first = static_cast<const uint8_t *>(d_px) + px_bytes * first;
        if ((rc = c.p_out.reserve(full * nb))) return rc;
        std::vector<PngSegment> segs(nb);
        BatchTail tail;
        tail.d_data = c.p_out.p;
        Stopwatch watch; // (debug switch trace: wall time between the host's waits)
        for (uint32_t i = 0; i < nb; ++i) { segs[i].src = full * i; segs[i].width = o.width; segs[i].height = o.height; }
        if (filter_batch) {
            for (PngSegment &sg : segs) {
                std::memset(&sg.layout, 0, sizeof(sg.layout));
                sg.layout.color_type_byte = o.color_type == PIXO_GRAY ? 0 : o.color_type == PIXO_GRAY_ALPHA ? 4 : o.color_type == PIXO_RGB ? 2 : 6;
                sg.layout.bit_depth = 8;
                sg.layout.bytes_per_pixel = static_cast<uint8_t>(bpp);
                sg.layout.row_bytes = o.width * bpp;
                sg.len = full;
                sg.view = PngFilterView{bpp, o.width * bpp + 1};
            }
            // filters, row sums on their way down, DEFLATE behind them: one wait for all three, then the checksums on the host
            if ((rc = png_filter_batch_begin(c, d_first, o.width, o.height, nb, bpp, run, c.p_out.p)) || (rc = tail_begin(c, segs, o.compression_level, png_effort(o), tail)) ||
                (rc = wait_for(c, sink)))
                return rc;
            for (uint32_t i = 0; i < nb; ++i) segs[i].adler = png_filter_batch_adler(c, static_cast<uint64_t>(i) * o.height, o.height, static_cast<uint64_t>(o.width) * bpp);
            watch.lap("png batch: filters, DEFLATE");
        } else {
            for (uint32_t i = 0; i < nb; ++i)
                if ((rc = png_segment_of_image(c, d_first + px_bytes * i, o, q, segs[i]))) return rc;
            watch.lap("png batch: images prepared");
            if ((rc = tail_begin(c, segs, o.compression_level, png_effort(o), tail))) return rc;
        }
        if ((rc = tail_finish(c, segs, tail, filter_batch)) || (rc = wait_for(c, sink))) return rc;
        watch.lap(filter_batch ? "png batch: scan, compact, CRC" : "png batch: DEFLATE to CRC");
        if ((rc = tail_deliver(c, segs, tail, first, sink))) return rc;
        watch.lap("png batch: copies, frames");
        if (debug().trace)
            std::fprintf(stderr, "[pixo_hip] png batch: sub-batch %u, %u image(s), %u chunk(s), %s way in, host waits %u%s\n", part, nb, tail.chunks,
                         filter_batch ? "batched" : "image-by-image", sink.waits - waits0, filter_batch ? "" : " (behind the images' own)");
    }
    return PIXO_OK;
}

int png_batch_blocks(Context &c, const void *d_px, const pixo_png_options &o, const pixo_png_quantization *q, uint32_t batch, uint8_t **files, size_t *lens)
{
    for (uint32_t i = 0; i < batch; ++i) { files[i] = nullptr; lens[i] = 0; }
    BatchSink sink;
    sink.files = files;
    sink.lens = lens;
    const int rc = png_batch(c, d_px, o, q, batch, sink);
    if (rc) {
        (void)hipStreamSynchronize(c.stream); // (no copy is in flight when the blocks go back)
        for (uint32_t i = 0; i < batch; ++i) { free_file(files[i]); files[i] = nullptr; lens[i] = 0; }
    }
    return rc;
}

int png_batch_into(Context &c, const void *d_px, const pixo_png_options &o, const pixo_png_quantization *q, uint32_t batch, uint8_t *arena,
                   size_t capacity, size_t *offsets, size_t *lens)
{
    for (uint32_t i = 0; i < batch; ++i) { offsets[i] = 0; lens[i] = 0; }
    BatchSink sink;
    sink.arena = arena;
    sink.cap = arena ? capacity : 0;
    sink.offsets = offsets;
    sink.lens = lens;
    const hipMemoryType arena_type = arena ? pointer_info(arena).type : hipMemoryTypeUnregistered;
    if (arena_type == hipMemoryTypeDevice) return hip_fail(hipErrorInvalidValue, "arena of a PNG batch in device memory (host memory only)");
    sink.pinned = arena_type == hipMemoryTypeHost;
    const int rc = png_batch(c, d_px, o, q, batch, sink);
    if (rc) return rc;
    return arena && sink.at <= capacity ? PIXO_OK : too_small(sink.at);
}

// The checks the three batch entries share behind png_check_options, in their order
int png_batch_checks(const void *pixels, uint32_t batch, const pixo_png_quantization *quantization, const void *files_or_offsets, const void *lens, bool into)
{
    PIXO_REQUIRE(pixels);
    int rc = batch_in_range(batch);
    if (rc || (quantization && (rc = png_check_quantization(quantization)))) return rc;
    if (into) { const void *offsets = files_or_offsets; PIXO_REQUIRE(offsets); }
    else { const void *files = files_or_offsets; PIXO_REQUIRE(files); }
    PIXO_REQUIRE(lens);
    return PIXO_OK;
}

// ---- images of individual sizes and colour types in one block ("Images of individual sizes") ----------
// What the driver decides about a batch before anything touches a device (also: pixo_hip_debug_png_encode_images_plan).
struct ImagesPlan {
    struct Image {
        pixo_png_options o; // the template with the image's width, height and colour type written into it
        uint32_t bpp = 0;
        size_t full = 0;    // h * (w * bpp + 1): its unreduced stream, what its segment is given
        int run = 0;        // what png_plan resolves for the unreduced image
        bool batched = false; // the batched way in: a ragged filter launch; otherwise png_segment_of_image
    };
    std::vector<Image> image;
    SubBatches sub_first;
};
// Sub-batches: greedy in index order under 64 MiB of unreduced stream (debug switch png_batch_bytes) and kBatchChunks chunks,
// at least one image each.  The way in is the image's own: png_plan with ITS area and height (an area of at most 4096 pixels
// turns the adaptive strategies into Sub, a height of at most 32 makes AdaptiveFast the sequential form).
int plan_images(const pixo_png_image *images, uint32_t batch, const pixo_png_options &o, const pixo_png_quantization *q, ImagesPlan &p)
{
    const uint64_t limit = debug().png_batch_bytes ? debug().png_batch_bytes : (uint64_t{64} << 20);
    p.image.resize(batch);
    uint64_t bytes = 0, chunks = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        ImagesPlan::Image &x = p.image[i];
        x.o = o;
        x.o.width = images[i].width;
        x.o.height = images[i].height;
        x.o.color_type = images[i].color_type;
        x.bpp = bytes_per_pixel(x.o.color_type);
        x.full = static_cast<size_t>(x.o.height) * (static_cast<size_t>(x.o.width) * x.bpp + 1);
        bool seq = false;
        if (const int rc = png_plan(x.o.width, x.o.height, static_cast<uint64_t>(x.o.width) * x.o.height, x.bpp, o.filter_strategy, o.flags, &x.run, &seq)) return rc;
        x.batched = !q && !o.optimize_alpha && !o.reduce_color_type && !o.reduce_palette && !seq;
        const uint64_t c = seg_chunks(x.full);
        if (p.sub_first.starts_at(i, bytes + x.full > limit || chunks + c > kBatchChunks)) bytes = chunks = 0;
        bytes += x.full;
        chunks += c;
    }
    p.sub_first.close(batch);
    return PIXO_OK;
}
// The items of a sub-batch's ragged launches: its batched images in index order, stream i at segment i's place.
std::vector<pixo_png_images::Item> items_of(const ImagesPlan &p, const pixo_png_image *images, uint32_t first, uint32_t end)
{
    std::vector<pixo_png_images::Item> items;
    size_t at = 0;
    for (uint32_t i = first; i < end; at += p.image[i].full, ++i) {
        const ImagesPlan::Image &x = p.image[i];
        if (x.batched) items.push_back({i - first, images[i].offset, at, x.o.width * x.bpp, x.o.height, x.bpp, x.run});
    }
    return items;
}

// The images at d_px + images[i].offset -> their files into the sink.  Sub-batches run one after the other on the context.
// In a sub-batch the image-by-image segments are prepared first (each waits for the host on its own: reductions, the
// quantiser, the sequential AdaptiveFast's checksum), then the ragged filter launches of the others are enqueued, then ONE
// tail runs over all segments: the DEFLATE of the prepared images is already behind the filters when the host waits for the
// row sums.  (The other order — launches first — would let every image-by-image wait drain the filter launches too, and
// both use the context's row sums.)
int png_images(Context &c, const void *d_px, const pixo_png_image *images, const pixo_png_options &o, const pixo_png_quantization *q, uint32_t batch,
               BatchSink &sink)
{
    ImagesPlan p;
    int rc = plan_images(images, batch, o, q, p);
    if (rc) return rc;
    const uint32_t subs = p.sub_first.count();
    note_route(route::PNG_IMAGES | (subs > 1 ? route::SUB_BATCHES : 0));
    for (uint32_t part = 0; part < subs; ++part) {
        const uint32_t first = p.sub_first[part], end = p.sub_first[part + 1], nb = end - first, waits0 = sink.waits;
        std::vector<PngSegment> segs(nb);
        size_t total = 0;
        for (uint32_t i = 0; i < nb; ++i) {
            segs[i].src = total;
            segs[i].width = p.image[first + i].o.width;
            segs[i].height = p.image[first + i].o.height;
            total += p.image[first + i].full;
        }
        if ((rc = c.p_out.reserve(total))) return rc;
        BatchTail tail;
        Stopwatch watch; // (debug switch trace: wall time between the host's waits)
        for (uint32_t i = 0; i < nb; ++i) {
            const ImagesPlan::Image &x = p.image[first + i];
            if (!x.batched && (rc = png_segment_of_image(c, static_cast<const uint8_t *>(d_px) + images[first + i].offset, x.o, q, segs[i]))) return rc;
        }
        watch.lap("png images: images prepared");
        tail.d_data = c.p_out.p; // (reserved for all streams before the first: nothing has moved)
        const std::vector<pixo_png_images::Item> items = items_of(p, images, first, end);
        uint32_t launches = 0;
        if (!items.empty()) {
            for (const pixo_png_images::Item &it : items) {
                const ImagesPlan::Image &x = p.image[first + it.image];
                PngSegment &sg = segs[it.image];
                std::memset(&sg.layout, 0, sizeof(sg.layout));
                sg.layout.color_type_byte = x.o.color_type == PIXO_GRAY ? 0 : x.o.color_type == PIXO_GRAY_ALPHA ? 4 : x.o.color_type == PIXO_RGB ? 2 : 6;
                sg.layout.bit_depth = 8;
                sg.layout.bytes_per_pixel = static_cast<uint8_t>(x.bpp);
                sg.layout.row_bytes = it.row_bytes;
                sg.len = x.full;
                sg.view = PngFilterView{x.bpp, it.row_bytes + 1};
            }
            note_route(route::PNG_IMAGES_FILTER);
            // filters, row sums on their way down, DEFLATE behind them: one wait for all three, then the checksums on the host
            if ((rc = png_filter_images_begin(c, d_px, items, c.p_out.p, &launches)) || (rc = tail_begin(c, segs, o.compression_level, png_effort(o), tail)) ||
                (rc = wait_for(c, sink)))
                return rc;
            uint64_t sums_at = 0;
            for (const pixo_png_images::Item &it : items) {
                segs[it.image].adler = png_filter_batch_adler(c, sums_at, it.height, it.row_bytes);
                sums_at += it.height;
            }
            watch.lap("png images: filters, DEFLATE");
        } else if ((rc = tail_begin(c, segs, o.compression_level, png_effort(o), tail))) {
            return rc;
        }
        if ((rc = tail_finish(c, segs, tail, !items.empty())) || (rc = wait_for(c, sink))) return rc;
        watch.lap("png images: scan, compact, CRC");
        if ((rc = tail_deliver(c, segs, tail, first, sink))) return rc;
        watch.lap("png images: copies, frames");
        if (debug().trace)
            std::fprintf(stderr, "[pixo_hip] png images: sub-batch %u, %u image(s), %u chunk(s), %zu batched in %u filter launch(es), host waits %u\n", part, nb,
                         tail.chunks, items.size(), launches, sink.waits - waits0);
    }
    return PIXO_OK;
}

int png_images_blocks(Context &c, const void *d_px, const pixo_png_image *images, const pixo_png_options &o, const pixo_png_quantization *q, uint32_t batch,
                      uint8_t **files, size_t *lens)
{
    for (uint32_t i = 0; i < batch; ++i) { files[i] = nullptr; lens[i] = 0; }
    BatchSink sink;
    sink.files = files;
    sink.lens = lens;
    const int rc = png_images(c, d_px, images, o, q, batch, sink);
    if (rc) {
        (void)hipStreamSynchronize(c.stream); // (no copy is in flight when the blocks go back)
        for (uint32_t i = 0; i < batch; ++i) { free_file(files[i]); files[i] = nullptr; lens[i] = 0; }
    }
    return rc;
}

int png_images_into(Context &c, const void *d_px, const pixo_png_image *images, const pixo_png_options &o, const pixo_png_quantization *q, uint32_t batch,
                    uint8_t *arena, size_t capacity, size_t *offsets, size_t *lens)
{
    for (uint32_t i = 0; i < batch; ++i) { offsets[i] = 0; lens[i] = 0; }
    BatchSink sink;
    sink.arena = arena;
    sink.cap = arena ? capacity : 0;
    sink.offsets = offsets;
    sink.lens = lens;
    const hipMemoryType arena_type = arena ? pointer_info(arena).type : hipMemoryTypeUnregistered;
    if (arena_type == hipMemoryTypeDevice) return hip_fail(hipErrorInvalidValue, "arena of a PNG batch in device memory (host memory only)");
    sink.pinned = arena_type == hipMemoryTypeHost;
    const int rc = png_images(c, d_px, images, o, q, batch, sink);
    if (rc) return rc;
    return arena && sink.at <= capacity ? PIXO_OK : too_small(sink.at);
}

// The checks the images entries share, in their order (include/pixo_hip.h): those in front of the out-pointers, then (behind
// them) every image's own; *block_end: the furthest image's end.  with_pixels false: the plan entry, which takes none.
int png_images_checks(const pixo_png_options *options, const void *pixels, bool with_pixels, const pixo_png_image *images, uint32_t batch,
                      const pixo_png_quantization *quantization)
{
    PIXO_REQUIRE(options);
    if (options->filter_strategy > PIXO_PNG_BIGRAMS) return fail(PIXO_ERR_COMPRESSION, "Compression error: unknown PNG filter strategy");
    if (with_pixels) PIXO_REQUIRE(pixels);
    PIXO_REQUIRE(images);
    int rc = batch_in_range(batch);
    if (rc || (quantization && (rc = png_check_quantization(quantization)))) return rc;
    return PIXO_OK;
}
int png_images_check_each(const pixo_png_image *images, uint32_t batch, uint64_t *block_end)
{
    *block_end = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        const pixo_png_image &im = images[i];
        int rc = png_check_image(im.width, im.height, im.color_type);
        if (rc) return fail(rc, t_error + where(i));
        if ((rc = record_extent(im.offset, image_bytes(im), "input", where(i), block_end))) return rc;
    }
    return PIXO_OK;
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
    BatchSink sink; // (the host waits twice: for the chunks' records, for the stream)
    if ((rc = zlib_stream(c, c.p_in.p, len, level, hint_bpp, hint_row, effort, nullptr, sink, &n)) || (rc = c.h_file.reserve(n))) return rc;
    HIP_TRY(hipMemcpyAsync(c.h_file.p, c.z_stream.p, n, hipMemcpyDeviceToHost, c.stream));
    if ((rc = wait_for(c, sink))) return rc;
    if (debug().trace) std::fprintf(stderr, "[pixo_hip] zlib: host waits %u\n", sink.waits);
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
    BatchSink sink; // (the host waits twice: for the chunks' records, for the stream)
    if ((rc = zlib_stream(*c, d_data, len, level, hint_bpp, hint_row, effort, d_out, sink, &n)) || (rc = wait_for(*c, sink))) return rc;
    if (debug().trace) std::fprintf(stderr, "[pixo_hip] zlib to the device: host waits %u\n", sink.waits);
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
    return png_file(c, c.p_in.p, *options, nullptr, out, out_len);
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
    return png_file(*c, d_pixels, *options, nullptr, out, out_len);
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
    return png_file(c, c.p_in.p, *options, quantization, out, out_len);
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
    return png_file(*c, d_pixels, *options, quantization, out, out_len);
}

int pixo_hip_png_encode_batch_device(const void *d_pixels, const pixo_png_options *options, const pixo_png_quantization *quantization, uint32_t batch,
                                     uint8_t **files, size_t *lens)
{
    int rc = png_check_options(options);
    if (rc || (rc = png_batch_checks(d_pixels, batch, quantization, files, lens, false))) return rc;
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return png_batch_blocks(*c, d_pixels, *options, quantization, batch, files, lens);
}

int pixo_hip_png_encode_batch_device_into(const void *d_pixels, const pixo_png_options *options, const pixo_png_quantization *quantization,
                                          uint32_t batch, uint8_t *arena, size_t capacity, size_t *offsets, size_t *lens)
{
    CallerStorageScope storage(arena && capacity);
    int rc = png_check_options(options);
    if (rc || (rc = png_batch_checks(d_pixels, batch, quantization, offsets, lens, true))) return rc;
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return png_batch_into(*c, d_pixels, *options, quantization, batch, arena, capacity, offsets, lens);
}

int pixo_hip_png_encode_batch(const uint8_t *data, size_t data_len, const pixo_png_options *options, const pixo_png_quantization *quantization,
                              uint32_t batch, uint8_t **files, size_t *lens)
{
    int rc = png_check_options(options, true, data_len, batch);
    if (rc) return rc;
    if ((rc = png_batch_checks(data, batch, quantization, files, lens, false))) return rc;
    PIXO_THREAD_CONTEXT(c);
    if ((rc = upload(c, c.p_in, data, data_len))) return rc;
    return png_batch_blocks(c, c.p_in.p, *options, quantization, batch, files, lens);
}

int pixo_hip_png_encode_images_device(const void *d_pixels, const pixo_png_image *images, uint32_t batch, const pixo_png_options *options,
                                      const pixo_png_quantization *quantization, uint8_t **files, size_t *lens)
{
    uint64_t end = 0;
    int rc = png_images_checks(options, d_pixels, true, images, batch, quantization);
    if (rc) return rc;
    PIXO_REQUIRE(files);
    PIXO_REQUIRE(lens);
    if ((rc = png_images_check_each(images, batch, &end))) return rc;
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return png_images_blocks(*c, d_pixels, images, *options, quantization, batch, files, lens);
}

int pixo_hip_png_encode_images_device_into(const void *d_pixels, const pixo_png_image *images, uint32_t batch, const pixo_png_options *options,
                                           const pixo_png_quantization *quantization, uint8_t *arena, size_t capacity, size_t *offsets, size_t *lens)
{
    CallerStorageScope storage(arena && capacity);
    uint64_t end = 0;
    int rc = png_images_checks(options, d_pixels, true, images, batch, quantization);
    if (rc) return rc;
    PIXO_REQUIRE(offsets);
    PIXO_REQUIRE(lens);
    if ((rc = png_images_check_each(images, batch, &end))) return rc;
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return png_images_into(*c, d_pixels, images, *options, quantization, batch, arena, capacity, offsets, lens);
}

int pixo_hip_png_encode_images(const uint8_t *data, size_t data_len, const pixo_png_image *images, uint32_t batch, const pixo_png_options *options,
                               const pixo_png_quantization *quantization, uint8_t **files, size_t *lens)
{
    uint64_t end = 0;
    int rc = png_images_checks(options, data, true, images, batch, quantization);
    if (rc) return rc;
    PIXO_REQUIRE(files);
    PIXO_REQUIRE(lens);
    if ((rc = png_images_check_each(images, batch, &end))) return rc;
    if (data_len < end) return bad_length(static_cast<size_t>(end), data_len);
    PIXO_THREAD_CONTEXT(c);
    if ((rc = upload(c, c.p_in, data, static_cast<size_t>(end)))) return rc;
    return png_images_blocks(c, c.p_in.p, images, *options, quantization, batch, files, lens);
}

int pixo_hip_debug_png_encode_images_plan(const pixo_png_image *images, uint32_t batch, const pixo_png_options *options,
                                          const pixo_png_quantization *quantization, uint32_t alignment, uint32_t *sub_first, uint32_t *sub_count,
                                          uint8_t *way_in, uint8_t *run_strategy, uint32_t *filter_launches)
{
    uint64_t end = 0;
    int rc = png_images_checks(options, nullptr, false, images, batch, quantization);
    if (rc) return rc;
    if (alignment > 15) return fail(PIXO_ERR_COMPRESSION, "Compression error: alignment must be 0..15");
    PIXO_REQUIRE(sub_first);
    PIXO_REQUIRE(sub_count);
    PIXO_REQUIRE(way_in);
    PIXO_REQUIRE(run_strategy);
    PIXO_REQUIRE(filter_launches);
    if ((rc = png_images_check_each(images, batch, &end))) return rc;
    ImagesPlan p;
    if ((rc = plan_images(images, batch, *options, quantization, p))) return rc;
    const uint32_t subs = p.sub_first.count();
    p.sub_first.report(sub_first, sub_count);
    *filter_launches = 0;
    for (uint32_t i = 0; i < batch; ++i) { way_in[i] = p.image[i].batched ? 1 : 0; run_strategy[i] = static_cast<uint8_t>(p.image[i].run); }
    for (uint32_t k = 0; k < subs; ++k) {
        std::vector<pixo_png_images::Record> table;
        std::vector<pixo_png_images::Launch> launches;
        std::vector<uint32_t> record_item;
        if (!pixo_png_images::build_table(items_of(p, images, p.sub_first[k], p.sub_first[k + 1]), alignment, table, launches, record_item))
            return hip_fail(hipErrorInvalidValue, "rows of a PNG batch");
        *filter_launches += static_cast<uint32_t>(launches.size());
    }
    return PIXO_OK;
}

} // extern "C"
