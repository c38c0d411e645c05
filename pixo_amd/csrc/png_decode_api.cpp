// png_decode_api.cpp — the extern "C" PNG decode entry points (pixo::decode::decode_png, reference src/decode/png.rs:101-291):
// the chunk walk and its checks in the reference's order and words, the host inflate (png_inflate.cpp) into pinned memory, the
// runs of rows that do not read the row above, and the launches of png_unfilter.hip.  The batch entries (N files -> N images
// back to back in device memory): two phases of checks, the inflates on a small pool of host threads, the plan of sub-batches
// and launches, one upload of streams and one of tables.  With PIXO_DECODE_DEVICE_INFLATE the batch entries inflate on the device
// (png_inflate.hip): the compressed streams go up, the host reads each stream's status and filter bytes and inflates again only
// what the device did not vouch for.
//
// The order in which a faulty file is refused: signature; per chunk in file order "truncated PNG chunk", its CRC-32, then its
// own length / field checks; then missing IEND, missing IHDR, zero dimension, dimension above 2^24, compression method, filter
// method, interlace (Unsupported), bit depth against colour type, no IDAT, whatever inflate raises, Adler-32, size, the first
// row in row order with a filter byte above 4, a palette image without PLTE.  All of it is known on the host before a kernel starts
// — except under PIXO_DECODE_DEVICE_INFLATE, where what follows the zlib header checks is known only behind the inflate launch of
// the file's sub-batch: d_pixels is unspecified after such a refusal (status, message and index are the same).
// The steps every batch driver takes, and their order: DESIGN.md §4.0; the shared ones: batch_steps.hpp.
#include "batch_steps.hpp"
#include "png_deflate_math.h"
#include "png_inflate.hpp"
#include "png_inflate_dev.hpp"
#include "png_unfilter.hpp"

#include <algorithm>
#include <atomic>

using namespace pixo_capi;
using namespace pixo_pngu;

namespace {

int invalid(const std::string &msg) { return fail(PIXO_ERR_INVALID_DECODE, "Decode error: " + msg); }
int unsupported(const std::string &msg) { return fail(PIXO_ERR_UNSUPPORTED_DECODE, "Unsupported: " + msg); }

// zlib.crc32, eight bytes a step
struct CrcTables {
    uint32_t t[8][256];
    CrcTables()
    {
        for (uint32_t i = 0; i < 256; ++i) t[0][i] = pixo_pngz::crc32_table_entry(i);
        for (uint32_t i = 0; i < 256; ++i)
            for (int k = 1; k < 8; ++k) t[k][i] = t[0][t[k - 1][i] & 255] ^ (t[k - 1][i] >> 8);
    }
};
uint32_t crc32_fast(const uint8_t *p, size_t n)
{
    static const CrcTables T;
    uint32_t c = 0xFFFFFFFFu;
    for (; n >= 8; n -= 8, p += 8) {
        uint32_t lo, hi;
        std::memcpy(&lo, p, 4);
        std::memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = T.t[7][lo & 255] ^ T.t[6][(lo >> 8) & 255] ^ T.t[5][(lo >> 16) & 255] ^ T.t[4][lo >> 24] ^ T.t[3][hi & 255] ^
            T.t[2][(hi >> 8) & 255] ^ T.t[1][(hi >> 16) & 255] ^ T.t[0][hi >> 24];
    }
    for (; n; --n, ++p) c = T.t[0][(c ^ *p) & 255] ^ (c >> 8);
    return ~c;
}

uint32_t be32(const uint8_t *p) { return (uint32_t{p[0]} << 24) | (uint32_t{p[1]} << 16) | (uint32_t{p[2]} << 8) | p[3]; }

// String::from_utf8_lossy of a chunk type: every maximal ill-formed run becomes U+FFFD
std::string utf8_lossy(const uint8_t *s, size_t n)
{
    std::string out;
    for (size_t i = 0; i < n;) {
        const uint8_t b = s[i];
        size_t need = 0;
        uint8_t lo = 0x80, hi = 0xBF;
        if (b < 0x80) { out += static_cast<char>(b); ++i; continue; }
        if (b >= 0xC2 && b <= 0xDF) need = 1;
        else if (b >= 0xE0 && b <= 0xEF) { need = 2; if (b == 0xE0) lo = 0xA0; if (b == 0xED) hi = 0x9F; }
        else if (b >= 0xF0 && b <= 0xF4) { need = 3; if (b == 0xF0) lo = 0x90; if (b == 0xF4) hi = 0x8F; }
        size_t got = 0;
        while (need && got < need && i + 1 + got < n) {
            const uint8_t c = s[i + 1 + got];
            if (c < (got == 0 ? lo : 0x80) || c > (got == 0 ? hi : 0xBF)) break;
            ++got;
        }
        if (need && got == need) out.append(reinterpret_cast<const char *>(s + i), need + 1);
        else out += "\xEF\xBF\xBD";
        i += 1 + got;
    }
    return out;
}

const char *color_type_name(uint32_t ct) // {:?} of PngColorType
{
    return ct == CT_GRAY ? "Grayscale" : ct == CT_RGB ? "Rgb" : ct == CT_INDEXED ? "Indexed" : ct == CT_GRAY_ALPHA ? "GrayscaleAlpha" : "Rgba";
}

struct PngFile {
    bool has_ihdr = false, has_plte = false, has_trns = false;
    uint32_t width = 0, height = 0;
    uint8_t depth = 0, color_type = 0, compression = 0, filter = 0, interlace = 0;
    const uint8_t *plte = nullptr, *trns = nullptr;
    uint32_t plte_entries = 0, trns_len = 0;
    // the IDAT bodies: one chunk is read where it lies, several are joined
    const uint8_t *idat = nullptr;
    size_t idat_len = 0, idat_chunks = 0;
    std::vector<uint8_t> joined;

    uint8_t out_color_type() const // png.rs:271-283
    {
        if (color_type == CT_GRAY) return PIXO_GRAY;
        if (color_type == CT_GRAY_ALPHA) return PIXO_GRAY_ALPHA;
        if (color_type == CT_RGBA) return PIXO_RGBA;
        return color_type == CT_INDEXED && has_trns && trns_has_alpha(trns, trns_len) ? PIXO_RGBA : PIXO_RGB;
    }
    uint64_t row_bytes() const { return pixo_pngu::row_bytes(color_type, depth, width); }
    size_t pixel_bytes() const { return static_cast<size_t>(width) * height * bytes_per_pixel(out_color_type()); }
};

// The walk (png.rs:102-205) and the checks behind it up to "no IDAT data" (:207-260).  join: the IDAT bodies are wanted.
int png_walk(const uint8_t *data, size_t len, bool join, PngFile &f)
{
    static const uint8_t kSignature[8] = {0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A};
    if (len < 8 || std::memcmp(data, kSignature, 8) != 0) return invalid("not a PNG file");
    size_t pos = 8;
    bool seen_iend = false;
    while (pos + 12 <= len) {
        const size_t length = be32(data + pos);
        const uint8_t *type = data + pos + 4, *body = data + pos + 8;
        if (length > len - pos - 12) return invalid("truncated PNG chunk"); // (pos + 12 <= len)
        if (be32(body + length) != crc32_fast(type, 4 + length)) return invalid("CRC mismatch in " + utf8_lossy(type, 4) + " chunk");
        if (!std::memcmp(type, "IHDR", 4)) {
            if (length != 13) return invalid("invalid IHDR length");
            const uint8_t ct = body[9];
            if (ct != CT_GRAY && ct != CT_RGB && ct != CT_INDEXED && ct != CT_GRAY_ALPHA && ct != CT_RGBA)
                return invalid("invalid PNG color type: " + std::to_string(ct));
            f.has_ihdr = true;
            f.width = be32(body); f.height = be32(body + 4);
            f.depth = body[8]; f.color_type = ct; f.compression = body[10]; f.filter = body[11]; f.interlace = body[12];
        } else if (!std::memcmp(type, "PLTE", 4)) {
            if (length % 3 != 0) return invalid("invalid PLTE length");
            f.has_plte = true; f.plte = body; f.plte_entries = static_cast<uint32_t>(length / 3);
        } else if (!std::memcmp(type, "tRNS", 4)) {
            f.has_trns = true; f.trns = body; f.trns_len = static_cast<uint32_t>(length);
        } else if (!std::memcmp(type, "IDAT", 4)) {
            if (join && length) {
                if (f.idat_chunks == 1) f.joined.assign(f.idat, f.idat + f.idat_len);
                if (f.idat_chunks >= 1) f.joined.insert(f.joined.end(), body, body + length);
                else f.idat = body;
                ++f.idat_chunks;
            }
            f.idat_len += length;
        } else if (!std::memcmp(type, "IEND", 4)) {
            seen_iend = true;
            break;
        }
        pos += 12 + length;
    }
    if (f.idat_chunks > 1) f.idat = f.joined.data();
    if (!seen_iend) return invalid("missing IEND chunk");
    if (!f.has_ihdr) return invalid("missing IHDR chunk");
    if (f.width == 0 || f.height == 0) return bad_dimensions(f.width, f.height);
    const uint32_t M = 1u << 24;
    if (f.width > M || f.height > M) return too_large(f.width, f.height, M);
    if (f.compression != 0) return invalid("unsupported compression method");
    if (f.filter != 0) return invalid("unsupported filter method");
    if (f.interlace != 0) return unsupported("Adam7 interlaced images not supported");
    if (!depth_valid(f.color_type, f.depth))
        return invalid("invalid bit depth " + std::to_string(f.depth) + " for color type " + color_type_name(f.color_type));
    if (f.idat_len == 0) return invalid("no IDAT data");
    return PIXO_OK;
}

int inflate_status(pixo_inflate::Kind k, const std::string &msg)
{
    return k == pixo_inflate::OK ? PIXO_OK : k == pixo_inflate::UNSUPPORTED ? unsupported(msg) : invalid(msg);
}

// The rows that do not read the row above (row 0, filter None or Sub) cut the image into segments; consecutive segments are
// joined into runs of at least kUnfilterPassRows rows (a run of short segments fills a wavefront's lanes), a run per workgroup.
struct Runs {
    std::vector<uint32_t> pairs; // (first row, rows)
    uint64_t segments = 0, longest_segment = 0;
};
// filters: row y's filter byte at filters[y * stride] (a stream: row_bytes + 1; the gathered bytes of the device inflate: 1).
// *bad_row: the first row whose filter byte is above 4 (height: none)
Runs find_runs(const uint8_t *filters, uint32_t height, uint64_t stride, uint32_t *bad_row)
{
    Runs r;
    *bad_row = height;
    uint32_t run_at = 0, seg_at = 0;
    for (uint32_t y = 0; y < height; ++y) {
        const uint8_t ft = filters[static_cast<size_t>(y) * stride];
        if (ft > FILTER_PAETH) { *bad_row = y; return r; }
        if (y > 0 && ft <= FILTER_SUB) {
            ++r.segments;
            r.longest_segment = std::max<uint64_t>(r.longest_segment, y - seg_at);
            seg_at = y;
            if (y - run_at >= pixo_dev::kUnfilterPassRows) {
                r.pairs.push_back(run_at);
                r.pairs.push_back(y - run_at);
                run_at = y;
            }
        }
    }
    ++r.segments;
    r.longest_segment = std::max<uint64_t>(r.longest_segment, height - seg_at);
    r.pairs.push_back(run_at);
    r.pairs.push_back(height - run_at);
    return r;
}

struct DecodeStats { // of the calling thread's last decode (tools/png_decode_timing.py)
    uint64_t segments = 0, longest_segment = 0, runs = 0;
    double walk_ms = 0, inflate_ms = 0, runs_ms = 0, upload_ms = 0, unfilter_ms = 0, convert_ms = 0;
};
thread_local DecodeStats t_stats;
struct Legs { // timed: events around the three device legs
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Legs() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

// Everything behind the walk: inflate into the context's pinned buffer, the checks that need the stream, upload, the two kernels
// on `s`, the pixels left at d_out (device memory of f.pixel_bytes() bytes).  Enqueue only; c.u_done is recorded behind the job.
int decode_on_device(Context &c, const PngFile &f, uint8_t *d_out, hipStream_t s, Legs *legs = nullptr)
{
    const uint64_t row = f.row_bytes(), pitch = pixo_dev::unfilter_pitch(row);
    const size_t expected = static_cast<size_t>(f.height) * (row + 1); // (2^24 rows of at most 2^27 + 1 bytes: fits 64 bits)
    int rc = await_last_job(c.u_done); // (it reads the pinned u_inflated and h_utables)
    if (rc) return rc;
    if ((rc = c.u_inflated.reserve(expected))) return rc;
    uint8_t *stream = c.u_inflated.as<uint8_t>();
    auto t0 = std::chrono::steady_clock::now();
    std::string msg;
    if ((rc = inflate_status(pixo_inflate::inflate_zlib(f.idat, f.idat_len, stream, expected, &msg), msg))) return rc;
    t_stats.inflate_ms = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    uint32_t bad_row = 0;
    const Runs runs = find_runs(stream, f.height, row + 1, &bad_row);
    if (bad_row < f.height) return invalid("invalid filter type: " + std::to_string(stream[static_cast<size_t>(bad_row) * (row + 1)]));
    if (f.color_type == CT_INDEXED && !f.has_plte) return invalid("missing PLTE chunk");
    t_stats.runs_ms = ms_since(t0);
    t_stats.segments = runs.segments; t_stats.longest_segment = runs.longest_segment; t_stats.runs = runs.pairs.size() / 2;

    // everything is reserved before any address is handed out
    const size_t table_bytes = 256 * sizeof(uint32_t), runs_bytes = runs.pairs.size() * sizeof(uint32_t);
    if ((rc = c.u_stream.reserve(pixo_dev::unfilter_stream_alloc(f.height, row))) || (rc = c.u_rows.reserve(static_cast<size_t>(f.height) * pitch)) ||
        (rc = c.h_utables.reserve(table_bytes + runs_bytes)) || (rc = c.u_tables.reserve(table_bytes + runs_bytes)))
        return rc;
    uint32_t *tables = c.h_utables.as<uint32_t>();
    const bool rgba = f.out_color_type() == PIXO_RGBA;
    for (uint32_t i = 0; i < 256; ++i) // (tRNS counts only where it holds a value other than 255: png.rs:501)
        tables[i] = f.color_type == CT_INDEXED ? palette_rgba(f.plte, f.plte_entries, f.trns, rgba ? f.trns_len : 0, i) : 0;
    std::memcpy(tables + 256, runs.pairs.data(), runs_bytes);

    if (legs) for (hipEvent_t &e : legs->e) HIP_TRY(hipEventCreate(&e));
    if (legs) HIP_TRY(hipEventRecord(legs->e[0], s));
    HIP_TRY(hipMemcpyAsync(c.u_stream.p, stream, expected, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c.u_tables.p, tables, table_bytes + runs_bytes, hipMemcpyHostToDevice, s));
    if (legs) HIP_TRY(hipEventRecord(legs->e[1], s));
    pixo_dev::UnfilterArgs u;
    u.stream = c.u_stream.as<uint8_t>(); u.rows = c.u_rows.as<uint8_t>();
    u.row_bytes = row; u.pitch = pitch; u.bpp = filter_unit(f.color_type, f.depth);
    u.runs = c.u_tables.as<uint32_t>() + 256; u.n_runs = static_cast<uint32_t>(runs.pairs.size() / 2);
    HIP_TRY(pixo_dev::launch_png_unfilter(u, s));
    if (legs) HIP_TRY(hipEventRecord(legs->e[2], s));
    pixo_dev::UnconvertArgs v;
    v.rows = u.rows; v.pitch = pitch; v.out = d_out; v.width = f.width; v.height = f.height;
    v.form = convert_of(f.color_type, f.depth); v.depth = f.depth; v.out_bpp = bytes_per_pixel(f.out_color_type());
    v.table = c.u_tables.as<uint32_t>();
    HIP_TRY(pixo_dev::launch_png_convert(v, s));
    if (legs) HIP_TRY(hipEventRecord(legs->e[3], s));
    HIP_TRY(hipEventRecord(c.u_done, s));
    return PIXO_OK;
}

void report_file(const PngFile &f, uint32_t *width, uint32_t *height, uint8_t *color_type)
{
    *width = f.width; *height = f.height; *color_type = f.out_color_type();
}

// Host file -> a block of the pinned pool the caller owns
int decode_to_block(const uint8_t *file, size_t len, uint8_t **pixels, size_t *pixels_len, uint32_t *width, uint32_t *height, uint8_t *color_type,
                    double *legs_ms)
{
    PngFile f;
    auto t0 = std::chrono::steady_clock::now();
    int rc = png_walk(file, len, true, f);
    if (rc) return rc;
    t_stats.walk_ms = ms_since(t0);
    PIXO_THREAD_CONTEXT(c);
    const size_t n = f.pixel_bytes();
    if ((rc = reserve16(c.u_out, n))) return rc;
    Legs legs;
    if ((rc = decode_on_device(c, f, c.u_out.as<uint8_t>(), c.stream, legs_ms ? &legs : nullptr))) return rc;
    if ((rc = download_pooled(c, c.u_out.p, n, "png decode", pixels, pixels_len))) return rc;
    if (legs_ms) {
        float ms = 0;
        for (int i = 0; i < 3; ++i) {
            HIP_TRY(hipEventElapsedTime(&ms, legs.e[i], legs.e[i + 1]));
            (i == 0 ? t_stats.upload_ms : i == 1 ? t_stats.unfilter_ms : t_stats.convert_ms) = ms;
        }
    }
    report_file(f, width, height, color_type);
    return PIXO_OK;
}

// ---- batches: N files -> N images back to back in HBM, one launch per pass and sub-batch (DESIGN.md §4.6e "Batches") ---------
constexpr uint64_t kDecodeBatchBytes = uint64_t{512} << 20; // device staging (streams + reconstructed rows) one sub-batch holds at most
                                                            // (debug switch decode_batch_bytes)
constexpr uint32_t kDecodeBatchThreads = 8;                 // host threads that inflate a batch, the caller among them, at most
constexpr uint32_t kFilterUnits[6] = {1, 2, 3, 4, 6, 8};

struct BatchFile {
    PngFile f;
    uint64_t row = 0, pitch = 0, expected = 0;
    uint64_t in_at = 0; // where its stream starts in the batch's staging (a multiple of 16)
    // phase 2, filled by whichever thread inflated the file
    pixo_inflate::Kind kind = pixo_inflate::OK;
    std::string msg;
    Runs runs;
};
struct DecodeBatch {
    std::vector<BatchFile> files;
    std::vector<pixo_png_image> images;
    uint64_t total = 0, staging = 0; // bytes of pixels (the end of the last image); bytes of all streams
    uint32_t threads = 1;
    double inflate_ms = 0;
};

// Phase 1 behind `files` and `batch`: per file its `data`, then the walk; the block's layout.  No HIP, no inflate.
int batch_walk(const pixo_png_file *files, uint32_t batch, bool join, DecodeBatch &b)
{
    b.files.resize(batch);
    b.images.resize(batch);
    for (uint32_t i = 0; i < batch; ++i) {
        if (!files[i].data) return fail(PIXO_ERR_COMPRESSION, "Compression error: null argument 'data'" + where(i));
        const int rc = png_walk(files[i].data, files[i].len, join, b.files[i].f);
        if (rc) return fail(rc, t_error + where(i));
    }
    uint64_t at = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        BatchFile &x = b.files[i];
        x.row = x.f.row_bytes();
        x.pitch = pixo_dev::unfilter_pitch(x.row);
        x.expected = static_cast<uint64_t>(x.f.height) * (x.row + 1);
        x.in_at = b.staging;
        b.staging += round16(x.expected);
        uint64_t end = 0; // (an image is at most 2^50 bytes: no wrap below the limit)
        const pixo_png_image im = lay_out(at, x.f.width, x.f.height, x.f.out_color_type(), &end);
        if (end > (uint64_t{1} << 62)) return fail(PIXO_ERR_COMPRESSION, "Compression error: batch output too large");
        b.images[i] = im;
        b.total = end;
    }
    return PIXO_OK;
}

// Phase 2: every stream inflated to stage + in_at and cut into runs, on up to kDecodeBatchThreads threads which hand back
// (kind, message) — fail() is the calling thread's; the failing file with the lowest index decides, whoever inflated it.
int batch_inflate(DecodeBatch &b, uint8_t *stage, uint32_t flags)
{
    const uint32_t batch = static_cast<uint32_t>(b.files.size());
    b.threads = (flags & PIXO_DECODE_ONE_THREAD) ? 1u : std::min(batch, kDecodeBatchThreads);
    const auto t0 = std::chrono::steady_clock::now();
    std::atomic<uint32_t> next{0};
    run_on_threads(b.threads, [&](unsigned) {
        for (uint32_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < batch;) {
            BatchFile &x = b.files[i];
            x.kind = pixo_inflate::inflate_zlib(x.f.idat, x.f.idat_len, stage + x.in_at, x.expected, &x.msg);
            if (x.kind != pixo_inflate::OK) continue;
            uint32_t bad_row = 0;
            x.runs = find_runs(stage + x.in_at, x.f.height, x.row + 1, &bad_row);
            if (bad_row < x.f.height) {
                x.kind = pixo_inflate::INVALID;
                x.msg = "invalid filter type: " + std::to_string(stage[x.in_at + static_cast<uint64_t>(bad_row) * (x.row + 1)]);
            } else if (x.f.color_type == CT_INDEXED && !x.f.has_plte) {
                x.kind = pixo_inflate::INVALID;
                x.msg = "missing PLTE chunk";
            }
        }
    });
    b.inflate_ms = ms_since(t0);
    for (uint32_t i = 0; i < batch; ++i)
        if (const int rc = inflate_status(b.files[i].kind, b.files[i].msg)) return fail(rc, t_error + where(i));
    return PIXO_OK;
}

// What the driver decided, before anything touches a device (also: pixo_hip_debug_png_decode_batch_plan)
struct DecodeBatchPlan {
    SubBatches sub_first;
    std::vector<uint64_t> rows_at;          // per image: its rows' offset in its sub-batch's rows buffer
    std::vector<uint32_t> kernel;           // per image: the convert kernel form (pixo_dev::ConvertKernel)
    uint64_t stream_bytes = 0, rows_bytes = 0; // the largest sub-batch's
    struct Unfilter { uint32_t sub, unit; uint64_t first_run, n_runs; };
    struct Convert { uint32_t sub, kernel; uint64_t first, n, max_items; };
    std::vector<Unfilter> unfilter;         // the launches in stream order within their sub-batch ...
    std::vector<Convert> convert;
    std::vector<pixo_dev::UnfilterBatchRun> runs; // ... and the tables they read: runs by (sub-batch, filter unit),
    std::vector<uint32_t> list;                   //     block tables by (sub-batch, kernel form)
};
// d_pixels: the address the offsets count from (the plan entry: 0, any 16-byte aligned block)
void decode_batch_plan(const DecodeBatch &b, uintptr_t d_pixels, DecodeBatchPlan &p)
{
    const uint32_t batch = static_cast<uint32_t>(b.files.size());
    const uint64_t limit = debug().decode_batch_bytes ? debug().decode_batch_bytes : kDecodeBatchBytes;
    p.rows_at.assign(batch, 0);
    p.kernel.assign(batch, 0);
    uint64_t held = 0, rows = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        const BatchFile &x = b.files[i];
        const uint64_t mine = x.f.height * x.pitch, need = round16(x.expected) + mine;
        if (p.sub_first.starts_at(i, held + need > limit)) held = rows = 0;
        p.rows_at[i] = rows;
        rows += mine;
        held += need;
        p.rows_bytes = std::max(p.rows_bytes, rows);
        p.stream_bytes = std::max(p.stream_bytes, x.in_at + round16(x.expected) - b.files[p.sub_first.back()].in_at);
        p.kernel[i] = pixo_dev::convert_kernel_of(convert_of(x.f.color_type, x.f.depth), static_cast<uint64_t>(x.f.width) * bytes_per_pixel(x.f.out_color_type()),
                                                  d_pixels + static_cast<uintptr_t>(b.images[i].offset));
    }
    p.sub_first.close(batch);
    for (uint32_t k = 0; k + 1 < p.sub_first.size(); ++k) {
        const uint32_t first = p.sub_first[k], end = p.sub_first[k + 1];
        for (const uint32_t unit : kFilterUnits) {
            const uint64_t run0 = p.runs.size();
            for (uint32_t i = first; i < end; ++i) {
                if (filter_unit(b.files[i].f.color_type, b.files[i].f.depth) != unit) continue;
                const std::vector<uint32_t> &pairs = b.files[i].runs.pairs;
                for (size_t r = 0; r + 1 < pairs.size(); r += 2) p.runs.push_back({i, pairs[r], pairs[r + 1], 0});
            }
            if (p.runs.size() > run0) p.unfilter.push_back({k, unit, run0, p.runs.size() - run0});
        }
        for (uint32_t form = 0; form < pixo_dev::CONVERT_KERNELS; ++form) {
            const uint64_t at = p.list.size();
            uint64_t max_items = 0;
            for (uint32_t i = first; i < end; ++i) {
                if (p.kernel[i] != form) continue;
                const PngFile &f = b.files[i].f;
                const uint64_t bytes = f.pixel_bytes();
                max_items = std::max<uint64_t>(max_items, form == pixo_dev::CONVERT_KERNEL_COPY16 ? bytes / 16
                                                        : form == pixo_dev::CONVERT_KERNEL_BYTES ? (bytes + 3) / 4 : static_cast<uint64_t>(f.width) * f.height);
                p.list.push_back(i);
            }
            if (p.list.size() > at) p.convert.push_back({k, form, at, p.list.size() - at, max_items});
        }
    }
}

// The tables of a batch in the pinned staging: descriptions, runs, block tables, a palette table per palette image; every section
// starts at a multiple of 16.  Reserves every buffer the launches of a batch use: nothing has been handed out yet.
struct BatchTables {
    size_t runs_at = 0, list_at = 0, tables_at = 0, up_bytes = 0;
};
int batch_tables(Context &c, const DecodeBatch &b, const DecodeBatchPlan &p, const uint8_t *d_pixels, BatchTables &t)
{
    const uint32_t batch = static_cast<uint32_t>(b.files.size());
    int rc;
    uint32_t palettes = 0;
    for (const BatchFile &x : b.files) palettes += x.f.color_type == CT_INDEXED;
    const size_t images_bytes = static_cast<size_t>(batch) * sizeof(pixo_dev::UnfilterBatchImage), runs_at = images_bytes;
    const size_t list_at = runs_at + p.runs.size() * sizeof(pixo_dev::UnfilterBatchRun);
    const size_t tables_at = round16(list_at + p.list.size() * sizeof(uint32_t));
    const size_t up_bytes = tables_at + std::max<size_t>(palettes, 1) * 256 * sizeof(uint32_t);
    // everything is reserved before any address is handed out
    if ((rc = c.u_stream.reserve(p.stream_bytes + pixo_dev::kUnfilterPiece)) || (rc = c.u_rows.reserve(p.rows_bytes)) ||
        (rc = c.h_utables.reserve(up_bytes)) || (rc = c.u_tables.reserve(up_bytes)))
        return rc;
    uint8_t *stage = c.h_utables.as<uint8_t>();
    pixo_dev::UnfilterBatchImage *images = reinterpret_cast<pixo_dev::UnfilterBatchImage *>(stage);
    uint32_t *palette = reinterpret_cast<uint32_t *>(stage + tables_at);
    uint32_t table_at = 0, sub = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        const BatchFile &x = b.files[i];
        while (i >= p.sub_first[sub + 1]) ++sub;
        pixo_dev::UnfilterBatchImage &im = images[i];
        std::memset(&im, 0, sizeof im);
        im.stream_at = x.in_at - b.files[p.sub_first[sub]].in_at;
        im.rows_at = p.rows_at[i];
        im.row_bytes = x.row; im.pitch = x.pitch;
        im.out_at = b.images[i].offset;
        im.width = x.f.width; im.height = x.f.height;
        im.form = convert_of(x.f.color_type, x.f.depth); im.depth = x.f.depth; im.out_bpp = bytes_per_pixel(x.f.out_color_type());
        im.aligned4 = (reinterpret_cast<uintptr_t>(d_pixels) + b.images[i].offset) % 4 == 0;
        if (x.f.color_type != CT_INDEXED) continue;
        im.table_at = table_at;
        const bool rgba = x.f.out_color_type() == PIXO_RGBA;
        for (uint32_t k = 0; k < 256; ++k) palette[table_at + k] = palette_rgba(x.f.plte, x.f.plte_entries, x.f.trns, rgba ? x.f.trns_len : 0, k);
        table_at += 256;
    }
    if (!p.runs.empty()) std::memcpy(stage + runs_at, p.runs.data(), p.runs.size() * sizeof(pixo_dev::UnfilterBatchRun));
    if (!p.list.empty()) std::memcpy(stage + list_at, p.list.data(), p.list.size() * sizeof(uint32_t));
    t.runs_at = runs_at; t.list_at = list_at; t.tables_at = tables_at; t.up_bytes = up_bytes;
    return PIXO_OK;
}
// One conversion launch of the plan
int launch_convert(Context &c, const DecodeBatchPlan::Convert &cv, const BatchTables &t, uint8_t *d_pixels, hipStream_t s)
{
    const uint8_t *d_tables = c.u_tables.as<uint8_t>();
    pixo_dev::UnconvertBatchArgs v;
    v.rows = c.u_rows.as<uint8_t>(); v.out = d_pixels; v.images = reinterpret_cast<const pixo_dev::UnfilterBatchImage *>(d_tables);
    v.list = reinterpret_cast<const uint32_t *>(d_tables + t.list_at) + cv.first;
    v.n = static_cast<uint32_t>(cv.n); v.kernel = cv.kernel;
    v.tables = reinterpret_cast<const uint32_t *>(d_tables + t.tables_at); v.max_items = cv.max_items;
    HIP_TRY(pixo_dev::launch_png_convert_batch(v, s));
    return PIXO_OK;
}

int decode_batch_device_inflate(Context &c, DecodeBatch &b, uint32_t flags, uint8_t *d_pixels, hipStream_t s, BatchLegs *legs);

// Everything behind phase 1: waits for this thread's previous decode job (the call's one host wait), inflates into the pinned
// staging, checks what only the streams show, then enqueues on `s`: all tables in one copy; per sub-batch its streams in one
// copy, one unfilter launch per filter unit, one convert launch per kernel form.  Nothing is enqueued after a refusal.
int decode_batch_on_device(Context &c, DecodeBatch &b, uint32_t flags, uint8_t *d_pixels, hipStream_t s, BatchLegs *legs = nullptr)
{
    const uint32_t batch = static_cast<uint32_t>(b.files.size());
    int rc = await_last_job(c.u_done); // (it reads the pinned u_inflated, h_utables, h_zin and h_uruns)
    if (rc) return rc;
    if (flags & PIXO_DECODE_DEVICE_INFLATE) return decode_batch_device_inflate(c, b, flags, d_pixels, s, legs);
    if ((rc = c.u_inflated.reserve(b.staging))) return rc;
    if ((rc = batch_inflate(b, c.u_inflated.as<uint8_t>(), flags))) return rc;
    DecodeBatchPlan p;
    decode_batch_plan(b, reinterpret_cast<uintptr_t>(d_pixels), p);
    const uint32_t subs = p.sub_first.count();
    note_route(route::PNG_DECODE_BATCH | (subs > 1 ? route::SUB_BATCHES : 0));

    BatchTables t;
    if ((rc = batch_tables(c, b, p, d_pixels, t))) return rc;
    const size_t runs_at = t.runs_at, up_bytes = t.up_bytes;
    uint8_t *stage = c.h_utables.as<uint8_t>();

    const uint8_t *d_tables = c.u_tables.as<uint8_t>();
    const pixo_dev::UnfilterBatchImage *d_images = reinterpret_cast<const pixo_dev::UnfilterBatchImage *>(d_tables);
    HIP_TRY(hipMemcpyAsync(c.u_tables.p, stage, up_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c.u_done, s)); // (until the job's own record: whatever has been enqueued when a later step fails)
    size_t iu = 0, iv = 0;
    for (uint32_t k = 0; k < subs; ++k) {
        const uint64_t from = b.files[p.sub_first[k]].in_at;
        const uint64_t bytes = (p.sub_first[k + 1] < batch ? b.files[p.sub_first[k + 1]].in_at : b.staging) - from;
        if (legs && (rc = legs->mark(s))) return rc;
        HIP_TRY(hipMemcpyAsync(c.u_stream.p, c.u_inflated.as<uint8_t>() + from, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(c.u_done, s));
        if (legs && (rc = legs->mark(s))) return rc;
        for (; iu < p.unfilter.size() && p.unfilter[iu].sub == k; ++iu) {
            pixo_dev::UnfilterBatchArgs u;
            u.stream = c.u_stream.as<uint8_t>(); u.rows = c.u_rows.as<uint8_t>(); u.images = d_images;
            u.runs = reinterpret_cast<const pixo_dev::UnfilterBatchRun *>(d_tables + runs_at) + p.unfilter[iu].first_run;
            u.n_runs = static_cast<uint32_t>(p.unfilter[iu].n_runs); u.bpp = p.unfilter[iu].unit;
            HIP_TRY(pixo_dev::launch_png_unfilter_batch(u, s));
        }
        if (legs && (rc = legs->mark(s))) return rc;
        for (; iv < p.convert.size() && p.convert[iv].sub == k; ++iv)
            if ((rc = launch_convert(c, p.convert[iv], t, d_pixels, s))) return rc;
        if (legs && (rc = legs->mark(s))) return rc;
        HIP_TRY(hipEventRecord(c.u_done, s));
    }
    return PIXO_OK;
}

// ---- PIXO_DECODE_DEVICE_INFLATE ------------------------------------------------------------------------------------------------
// The zlib header checks of inflate_zlib (the 6-byte minimum, method, header checksum, preset dictionary): what the kernel never sees
bool zlib_head_sound(const PngFile &f)
{
    if (f.idat_len < 6) return false;
    const uint8_t cmf = f.idat[0], flg = f.idat[1];
    return (cmf & 0x0F) == 8 && ((static_cast<unsigned>(cmf) << 8) | flg) % 31 == 0 && !(flg & 0x20);
}
// Before a device is touched: a file whose zlib header is unsound makes the call end as it does without the flag — the host
// inflates into ordinary memory and the failing file with the lowest index decides, this one or one in front of it.
int batch_zlib_heads(DecodeBatch &b, uint32_t flags)
{
    bool sound = true;
    for (const BatchFile &x : b.files) sound = sound && zlib_head_sound(x.f);
    if (sound) return PIXO_OK;
    uint8_t *stage = static_cast<uint8_t *>(std::malloc(std::max<size_t>(static_cast<size_t>(b.staging), 1)));
    if (!stage) return fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
    const int rc = batch_inflate(b, stage, flags);
    std::free(stage);
    return rc ? rc : invalid("invalid zlib stream"); // (never: the host inflate makes the same header checks)
}

// A sub-batch's compressed streams in the pinned staging as the kernel wants them: every stream's DEFLATE bytes start at a
// multiple of 16 and are followed by at least 16 zero bytes.
inline uint64_t inflate_input_bytes(const PngFile &f) { return round16(f.idat_len - 6) + pixo_dev::kInflateInputAlign; }

// The batch job with the inflates on the device.  Per sub-batch: descriptions and compressed streams up in one copy, the inflate
// launch, the gather of the filter bytes, status records and filter bytes down in one copy, ONE host wait; then the host decides
// in index order (a stream the device does not vouch for is inflated again here: the host's result is the truth), the runs of
// rows go up, and the unfilter and convert launches follow as without the flag.  The wait for sub-batch k's records also covers
// everything enqueued before it, so the pinned staging (h_zin, h_uruns, u_inflated) is free to be rewritten for sub-batch k.
int decode_batch_device_inflate(Context &c, DecodeBatch &b, uint32_t flags, uint8_t *d_pixels, hipStream_t s, BatchLegs *legs)
{
    using pixo_dev::FilterGatherImage;
    using pixo_dev::InflateStatus;
    using pixo_dev::InflateStream;
    int rc;
    DecodeBatchPlan p; // (no runs are known yet: the cuts, the rows' places and the conversion launches do not need them)
    decode_batch_plan(b, reinterpret_cast<uintptr_t>(d_pixels), p);
    const uint32_t subs = p.sub_first.count();
    note_route(route::PNG_DECODE_BATCH | route::PNG_INFLATE_DEVICE | (subs > 1 ? route::SUB_BATCHES : 0));
    BatchTables t;
    if ((rc = batch_tables(c, b, p, d_pixels, t))) return rc;
    // the largest sub-batch's staging: descriptions + padded inputs; records + filter bytes; runs (a run but the last has pass_rows rows)
    size_t zin_bytes = 0, zout_bytes = 0, runs_bytes = 0;
    for (uint32_t k = 0; k < subs; ++k) {
        size_t in = 0, rows = 0, runs = 0;
        for (uint32_t i = p.sub_first[k]; i < p.sub_first[k + 1]; ++i) {
            in += inflate_input_bytes(b.files[i].f);
            rows += b.files[i].f.height;
            runs += b.files[i].f.height / pixo_dev::kUnfilterPassRows + 1;
        }
        const size_t m = p.sub_first[k + 1] - p.sub_first[k];
        zin_bytes = std::max(zin_bytes, m * (sizeof(InflateStream) + sizeof(FilterGatherImage)) + in);
        zout_bytes = std::max(zout_bytes, m * sizeof(InflateStatus) + rows);
        runs_bytes = std::max(runs_bytes, runs * sizeof(pixo_dev::UnfilterBatchRun));
    }
    if ((rc = c.h_zin.reserve(zin_bytes)) || (rc = c.u_zin.reserve(zin_bytes)) || (rc = c.u_zout.reserve(zout_bytes)) ||
        (rc = c.h_zout.reserve(zout_bytes)) || (rc = c.h_uruns.reserve(runs_bytes)) || (rc = c.u_runs.reserve(runs_bytes)))
        return rc;

    const uint8_t *d_tables = c.u_tables.as<uint8_t>();
    const pixo_dev::UnfilterBatchImage *h_images = c.h_utables.as<pixo_dev::UnfilterBatchImage>();
    HIP_TRY(hipMemcpyAsync(c.u_tables.p, c.h_utables.p, t.up_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c.u_done, s));
    b.threads = 1;
    size_t iv = 0;
    for (uint32_t k = 0; k < subs; ++k) {
        const uint32_t first = p.sub_first[k], end = p.sub_first[k + 1], m = end - first;
        const auto t0 = std::chrono::steady_clock::now();
        uint8_t *zin = c.h_zin.as<uint8_t>();
        InflateStream *streams = reinterpret_cast<InflateStream *>(zin);
        FilterGatherImage *gather = reinterpret_cast<FilterGatherImage *>(zin + m * sizeof(InflateStream));
        const size_t input_at = m * (sizeof(InflateStream) + sizeof(FilterGatherImage));
        uint64_t in_at = 0, filters_at = 0;
        uint32_t max_height = 0;
        for (uint32_t i = first; i < end; ++i) {
            const BatchFile &x = b.files[i];
            const uint64_t in_len = x.f.idat_len - 6, padded = inflate_input_bytes(x.f);
            streams[i - first] = {in_at, in_len, h_images[i].stream_at, x.expected};
            gather[i - first] = {h_images[i].stream_at, x.row + 1, filters_at, x.f.height, 0};
            std::memcpy(zin + input_at + in_at, x.f.idat + 2, in_len);
            std::memset(zin + input_at + in_at + in_len, 0, padded - in_len);
            in_at += padded;
            filters_at += x.f.height;
            max_height = std::max(max_height, x.f.height);
        }
        if (legs && (rc = legs->mark(s))) return rc;
        HIP_TRY(hipMemcpyAsync(c.u_zin.p, zin, input_at + in_at, hipMemcpyHostToDevice, s));
        pixo_dev::InflateArgs ia;
        ia.input = c.u_zin.as<uint8_t>() + input_at; ia.out = c.u_stream.as<uint8_t>();
        ia.streams = c.u_zin.as<InflateStream>(); ia.status = c.u_zout.as<InflateStatus>(); ia.n = m;
        HIP_TRY(pixo_dev::launch_png_inflate(ia, s));
        pixo_dev::FilterGatherArgs ga;
        ga.stream = c.u_stream.as<uint8_t>(); ga.filters = c.u_zout.as<uint8_t>() + m * sizeof(InflateStatus);
        ga.images = reinterpret_cast<const FilterGatherImage *>(c.u_zin.as<uint8_t>() + m * sizeof(InflateStream)); ga.n = m; ga.max_height = max_height;
        HIP_TRY(pixo_dev::launch_png_filter_gather(ga, s));
        HIP_TRY(hipMemcpyAsync(c.h_zout.p, c.u_zout.p, m * sizeof(InflateStatus) + filters_at, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(c.u_done, s));
        HIP_TRY(hipEventSynchronize(c.u_done)); // the sub-batch's one host wait
        const InflateStatus *status = c.h_zout.as<InflateStatus>();
        const uint8_t *filters = c.h_zout.as<uint8_t>() + m * sizeof(InflateStatus);

        // what the device does not vouch for is inflated again by the host, on the pool (or on the caller)
        std::vector<uint32_t> suspect;
        std::vector<uint64_t> redo_at;
        uint64_t redo_bytes = 0;
        for (uint32_t i = first; i < end; ++i) {
            const PngFile &f = b.files[i].f;
            if (status[i - first].verdict == pixo_pngi::OK && status[i - first].adler == be32(f.idat + f.idat_len - 4)) continue;
            suspect.push_back(i);
            redo_at.push_back(redo_bytes);
            redo_bytes += round16(b.files[i].expected);
        }
        if (!suspect.empty()) {
            if ((rc = c.u_inflated.reserve(redo_bytes))) return rc;
            const uint32_t threads = (flags & PIXO_DECODE_ONE_THREAD) ? 1u : std::min<uint32_t>(static_cast<uint32_t>(suspect.size()), kDecodeBatchThreads);
            b.threads = std::max(b.threads, threads);
            std::atomic<uint32_t> next{0};
            run_on_threads(threads, [&](unsigned) {
                for (uint32_t j; (j = next.fetch_add(1, std::memory_order_relaxed)) < suspect.size();) {
                    BatchFile &x = b.files[suspect[j]];
                    x.kind = pixo_inflate::inflate_zlib(x.f.idat, x.f.idat_len, c.u_inflated.as<uint8_t>() + redo_at[j], x.expected, &x.msg);
                }
            });
        }
        // ... and then, in index order, the checks in the order they have without the flag
        uint64_t at = 0;
        for (uint32_t i = first, j = 0; i < end; at += b.files[i].f.height, ++i) {
            BatchFile &x = b.files[i];
            const std::string here = where(i);
            const uint8_t *bytes = filters + at;
            uint64_t stride = 1;
            if (j < suspect.size() && suspect[j] == i) {
                if ((rc = inflate_status(x.kind, x.msg))) return fail(rc, t_error + here);
                bytes = c.u_inflated.as<uint8_t>() + redo_at[j];
                stride = x.row + 1;
                HIP_TRY(hipMemcpyAsync(c.u_stream.as<uint8_t>() + h_images[i].stream_at, bytes, x.expected, hipMemcpyHostToDevice, s));
                HIP_TRY(hipEventRecord(c.u_done, s));
                note_route(route::PNG_INFLATE_HOST_REDO);
                ++j;
            }
            uint32_t bad_row = 0;
            x.runs = find_runs(bytes, x.f.height, stride, &bad_row);
            if (bad_row < x.f.height) return fail(invalid("invalid filter type: " + std::to_string(bytes[bad_row * stride])), t_error + here);
            if (x.f.color_type == CT_INDEXED && !x.f.has_plte) return fail(invalid("missing PLTE chunk"), t_error + here);
        }
        // the runs of this sub-batch by filter unit, as decode_batch_plan lays them out
        pixo_dev::UnfilterBatchRun *runs = c.h_uruns.as<pixo_dev::UnfilterBatchRun>();
        struct Launch { uint32_t unit; size_t first_run, n_runs; };
        std::vector<Launch> launches;
        size_t n_runs = 0;
        for (const uint32_t unit : kFilterUnits) {
            const size_t run0 = n_runs;
            for (uint32_t i = first; i < end; ++i) {
                if (filter_unit(b.files[i].f.color_type, b.files[i].f.depth) != unit) continue;
                const std::vector<uint32_t> &pairs = b.files[i].runs.pairs;
                for (size_t r = 0; r + 1 < pairs.size(); r += 2) runs[n_runs++] = {i, pairs[r], pairs[r + 1], 0};
            }
            if (n_runs > run0) launches.push_back({unit, run0, n_runs - run0});
        }
        b.inflate_ms += ms_since(t0);
        HIP_TRY(hipMemcpyAsync(c.u_runs.p, runs, n_runs * sizeof(pixo_dev::UnfilterBatchRun), hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(c.u_done, s));
        if (legs && (rc = legs->mark(s))) return rc;
        for (const Launch &l : launches) {
            pixo_dev::UnfilterBatchArgs u;
            u.stream = c.u_stream.as<uint8_t>(); u.rows = c.u_rows.as<uint8_t>();
            u.images = reinterpret_cast<const pixo_dev::UnfilterBatchImage *>(d_tables);
            u.runs = c.u_runs.as<pixo_dev::UnfilterBatchRun>() + l.first_run;
            u.n_runs = static_cast<uint32_t>(l.n_runs); u.bpp = l.unit;
            HIP_TRY(pixo_dev::launch_png_unfilter_batch(u, s));
        }
        if (legs && (rc = legs->mark(s))) return rc;
        for (; iv < p.convert.size() && p.convert[iv].sub == k; ++iv)
            if ((rc = launch_convert(c, p.convert[iv], t, d_pixels, s))) return rc;
        if (legs && (rc = legs->mark(s))) return rc;
        HIP_TRY(hipEventRecord(c.u_done, s));
    }
    return PIXO_OK;
}

// The inflate kernel alone (pixo_hip_debug_zlib_inflate_batch_device)
int inflate_batch_debug(Context &c, const pixo_png_file *streams, uint32_t n, const uint64_t *expected, uint8_t *out, const uint64_t *out_at,
                        uint32_t *verdict, uint64_t *produced, uint32_t *adler, double *kernel_ms)
{
    using pixo_dev::InflateStatus;
    using pixo_dev::InflateStream;
    int rc;
    uint64_t block = 0, in_bytes = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!streams[i].data) return fail(PIXO_ERR_COMPRESSION, "Compression error: null argument 'data'" + where(i));
        if (streams[i].len < 6) return fail(invalid("zlib stream too short"), t_error + where(i));
        if (out_at[i] > (uint64_t{1} << 40) || expected[i] > (uint64_t{1} << 40)) return fail(PIXO_ERR_COMPRESSION, "Compression error: region too large" + where(i));
        block = std::max(block, out_at[i] + expected[i]);
        in_bytes += round16(streams[i].len - 6) + pixo_dev::kInflateInputAlign;
    }
    if (block) PIXO_REQUIRE(out);
    if ((rc = await_last_job(c.u_done))) return rc;
    const size_t input_at = static_cast<size_t>(n) * sizeof(InflateStream), status_bytes = static_cast<size_t>(n) * sizeof(InflateStatus);
    if ((rc = c.h_zin.reserve(input_at + in_bytes)) || (rc = c.u_zin.reserve(input_at + in_bytes)) || (rc = c.u_zout.reserve(status_bytes)) ||
        (rc = c.h_zout.reserve(status_bytes)) || (rc = c.u_stream.reserve(block + pixo_dev::kUnfilterPiece)))
        return rc;
    uint8_t *zin = c.h_zin.as<uint8_t>();
    uint64_t in_at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t in_len = streams[i].len - 6, padded = round16(in_len) + pixo_dev::kInflateInputAlign;
        reinterpret_cast<InflateStream *>(zin)[i] = {in_at, in_len, out_at[i], expected[i]};
        std::memcpy(zin + input_at + in_at, streams[i].data + 2, in_len);
        std::memset(zin + input_at + in_at + in_len, 0, padded - in_len);
        in_at += padded;
    }
    hipStream_t s = c.stream;
    Legs timed;
    for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreate(&timed.e[i]));
    HIP_TRY(hipMemcpyAsync(c.u_zin.p, zin, input_at + in_at, hipMemcpyHostToDevice, s));
    if (block) HIP_TRY(hipMemcpyAsync(c.u_stream.p, out, block, hipMemcpyHostToDevice, s));
    pixo_dev::InflateArgs ia;
    ia.input = c.u_zin.as<uint8_t>() + input_at; ia.out = c.u_stream.as<uint8_t>();
    ia.streams = c.u_zin.as<InflateStream>(); ia.status = c.u_zout.as<InflateStatus>(); ia.n = n;
    HIP_TRY(hipEventRecord(timed.e[0], s));
    HIP_TRY(pixo_dev::launch_png_inflate(ia, s));
    HIP_TRY(hipEventRecord(timed.e[1], s));
    HIP_TRY(hipMemcpyAsync(c.h_zout.p, c.u_zout.p, status_bytes, hipMemcpyDeviceToHost, s));
    if (block) HIP_TRY(hipMemcpyAsync(out, c.u_stream.p, block, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(c.u_done, s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, timed.e[0], timed.e[1]));
    *kernel_ms = ms;
    const InflateStatus *status = c.h_zout.as<InflateStatus>();
    for (uint32_t i = 0; i < n; ++i) { verdict[i] = status[i].verdict; produced[i] = status[i].produced; adler[i] = status[i].adler; }
    return PIXO_OK;
}

// Host files -> one block of the pinned pool the caller owns
int decode_batch_to_block(const pixo_png_file *files, uint32_t batch, uint32_t flags, uint8_t **out, size_t *out_len, pixo_png_image *images, double *legs_ms)
{
    DecodeBatch b;
    int rc = batch_walk(files, batch, true, b);
    if (rc) return rc;
    report(b.images, images);
    if ((flags & PIXO_DECODE_DEVICE_INFLATE) && (rc = batch_zlib_heads(b, flags))) return rc;
    PIXO_THREAD_CONTEXT(c);
    const size_t n = static_cast<size_t>(b.total);
    if ((rc = reserve16(c.u_out, n))) return rc;
    BatchLegs legs;
    if ((rc = decode_batch_on_device(c, b, flags, c.u_out.as<uint8_t>(), c.stream, legs_ms ? &legs : nullptr))) return rc;
    uint8_t *block = nullptr;
    size_t got = 0;
    if ((rc = download_pooled(c, c.u_out.p, n, "png decode batch", &block, &got))) return rc;
    if (legs_ms) {
        legs_ms[0] = b.inflate_ms;
        legs_ms[1] = legs_ms[2] = legs_ms[3] = 0;
        for (size_t k = 0; k + 3 < legs.e.size(); k += 4)
            for (int i = 0; i < 3; ++i) {
                float ms = 0;
                const hipError_t e = hipEventElapsedTime(&ms, legs.e[k + i], legs.e[k + i + 1]);
                if (e != hipSuccess) { free_file(block); return hip_fail(e, "hipEventElapsedTime"); }
                legs_ms[1 + i] += ms;
            }
    }
    *out = block;
    *out_len = got;
    return PIXO_OK;
}

} // namespace

extern "C" {

int pixo_hip_png_decode_batch_info(const pixo_png_file *files, uint32_t batch, pixo_png_image *images, size_t *total)
{
    int rc = batch_head(files, batch);
    if (rc) return rc;
    PIXO_REQUIRE(images);
    PIXO_REQUIRE(total);
    DecodeBatch b;
    if ((rc = batch_walk(files, batch, false, b))) return rc;
    report(b.images, images);
    *total = static_cast<size_t>(b.total);
    return PIXO_OK;
}

int pixo_hip_png_decode_batch_device(const pixo_png_file *files, uint32_t batch, uint32_t flags, void *d_pixels, size_t capacity,
                                     pixo_png_image *images, void *stream)
{
    CallerStorageScope storage(d_pixels != nullptr && capacity != 0);
    int rc = batch_head(files, batch);
    if (rc) return rc;
    PIXO_REQUIRE(images);
    DecodeBatch b;
    if ((rc = batch_walk(files, batch, true, b))) return rc;
    report(b.images, images);
    if (capacity < b.total) return too_small(static_cast<size_t>(b.total));
    PIXO_REQUIRE(d_pixels);
    if ((flags & PIXO_DECODE_DEVICE_INFLATE) && (rc = batch_zlib_heads(b, flags))) return rc;
    PIXO_CALLER_STREAM_CONTEXT(c, s, stream);
    return decode_batch_on_device(*c, b, flags, static_cast<uint8_t *>(d_pixels), s);
}

int pixo_hip_png_decode_batch(const pixo_png_file *files, uint32_t batch, uint32_t flags, uint8_t **out, size_t *out_len, pixo_png_image *images)
{
    const int rc = batch_head(files, batch);
    if (rc) return rc;
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    PIXO_REQUIRE(images);
    return decode_batch_to_block(files, batch, flags, out, out_len, images, nullptr);
}

int pixo_hip_debug_png_decode_batch_plan(const pixo_png_file *files, uint32_t batch, uint32_t flags, uint32_t *sub_first, uint32_t *sub_count,
                                         uint64_t *runs_per_image, uint32_t *unfilter_launches, uint32_t *convert_launches, uint32_t *threads)
{
    int rc = batch_head(files, batch);
    if (rc) return rc;
    PIXO_REQUIRE(sub_first);
    PIXO_REQUIRE(sub_count);
    PIXO_REQUIRE(runs_per_image);
    PIXO_REQUIRE(unfilter_launches);
    PIXO_REQUIRE(convert_launches);
    PIXO_REQUIRE(threads);
    DecodeBatch b;
    if ((rc = batch_walk(files, batch, true, b))) return rc;
    uint8_t *stage = static_cast<uint8_t *>(std::malloc(std::max<size_t>(static_cast<size_t>(b.staging), 1)));
    if (!stage) return fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
    rc = batch_inflate(b, stage, flags);
    std::free(stage);
    if (rc) return rc;
    DecodeBatchPlan p;
    decode_batch_plan(b, 0, p);
    p.sub_first.report(sub_first, sub_count);
    for (uint32_t i = 0; i < batch; ++i) runs_per_image[i] = b.files[i].runs.pairs.size() / 2;
    *unfilter_launches = static_cast<uint32_t>(p.unfilter.size());
    *convert_launches = static_cast<uint32_t>(p.convert.size());
    *threads = b.threads;
    return PIXO_OK;
}

int pixo_hip_debug_png_decode_batch_timed(const pixo_png_file *files, uint32_t batch, uint32_t flags, double ms[5])
{
    const int rc0 = batch_head(files, batch);
    if (rc0) return rc0;
    PIXO_REQUIRE(ms);
    uint8_t *block = nullptr;
    size_t n = 0;
    std::vector<pixo_png_image> images(batch);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = decode_batch_to_block(files, batch, flags, &block, &n, images.data(), ms);
    if (rc) return rc;
    ms[4] = ms_since(t0);
    free_file(block);
    return PIXO_OK;
}

int pixo_hip_png_decode(const uint8_t *file, size_t len, uint8_t **pixels, size_t *pixels_len, uint32_t *width, uint32_t *height, uint8_t *color_type)
{
    PIXO_REQUIRE(file);
    PIXO_REQUIRE(pixels);
    PIXO_REQUIRE(pixels_len);
    PIXO_REQUIRE(width);
    PIXO_REQUIRE(height);
    PIXO_REQUIRE(color_type);
    return decode_to_block(file, len, pixels, pixels_len, width, height, color_type, nullptr);
}

int pixo_hip_png_decode_info(const uint8_t *file, size_t len, uint32_t *width, uint32_t *height, uint8_t *color_type)
{
    PIXO_REQUIRE(file);
    PIXO_REQUIRE(width);
    PIXO_REQUIRE(height);
    PIXO_REQUIRE(color_type);
    PngFile f;
    const int rc = png_walk(file, len, false, f);
    if (rc) return rc;
    report_file(f, width, height, color_type);
    return PIXO_OK;
}

int pixo_hip_png_decode_device(const uint8_t *file, size_t len, void *d_pixels, size_t capacity, uint32_t *width, uint32_t *height,
                               uint8_t *color_type, void *stream)
{
    CallerStorageScope storage(d_pixels != nullptr && capacity != 0);
    PIXO_REQUIRE(file);
    PIXO_REQUIRE(width);
    PIXO_REQUIRE(height);
    PIXO_REQUIRE(color_type);
    PngFile f;
    int rc = png_walk(file, len, true, f);
    if (rc) return rc;
    report_file(f, width, height, color_type);
    if (capacity < f.pixel_bytes()) return too_small(f.pixel_bytes());
    PIXO_REQUIRE(d_pixels);
    PIXO_CALLER_STREAM_CONTEXT(c, s, stream);
    return decode_on_device(*c, f, static_cast<uint8_t *>(d_pixels), s);
}

int pixo_hip_zlib_inflate(const uint8_t *data, size_t len, uint8_t *out, size_t expected)
{
    PIXO_REQUIRE(data);
    if (expected) PIXO_REQUIRE(out);
    std::string msg;
    return inflate_status(pixo_inflate::inflate_zlib(data, len, out, expected, &msg), msg);
}

uint32_t pixo_hip_png_unfilter_pass_rows(void) { return pixo_dev::kUnfilterPassRows; }
uint32_t pixo_hip_png_inflate_step_tokens(void) { return pixo_pngi::kStepTokens; }
uint32_t pixo_hip_png_inflate_window_bytes(void) { return pixo_pngi::kWindowBytes; }
uint32_t pixo_hip_png_inflate_far_distance(void) { return pixo_pngi::kFarDistance; }
uint32_t pixo_hip_png_inflate_stored_chunk(void) { return pixo_pngi::kStoredChunk; }

int pixo_hip_debug_zlib_inflate_batch_device(const pixo_png_file *streams, uint32_t n, const uint64_t *expected, uint8_t *out, const uint64_t *out_at,
                                             uint32_t *verdict, uint64_t *produced, uint32_t *adler, double *kernel_ms)
{
    PIXO_REQUIRE(streams);
    const int rc = batch_in_range(n);
    if (rc) return rc;
    PIXO_REQUIRE(expected);
    PIXO_REQUIRE(out_at);
    PIXO_REQUIRE(verdict);
    PIXO_REQUIRE(produced);
    PIXO_REQUIRE(adler);
    PIXO_REQUIRE(kernel_ms);
    PIXO_THREAD_CONTEXT(c);
    return inflate_batch_debug(c, streams, n, expected, out, out_at, verdict, produced, adler, kernel_ms);
}

int pixo_hip_debug_png_decode_timed(const uint8_t *file, size_t len, double ms[7], uint64_t counts[3])
{
    PIXO_REQUIRE(file);
    PIXO_REQUIRE(ms);
    PIXO_REQUIRE(counts);
    uint8_t *pixels = nullptr;
    size_t n = 0;
    uint32_t w = 0, h = 0;
    uint8_t ct = 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = decode_to_block(file, len, &pixels, &n, &w, &h, &ct, ms);
    if (rc) return rc;
    const double whole = ms_since(t0);
    free_file(pixels);
    const DecodeStats &t = t_stats;
    ms[0] = t.walk_ms; ms[1] = t.inflate_ms; ms[2] = t.runs_ms; ms[3] = t.upload_ms; ms[4] = t.unfilter_ms; ms[5] = t.convert_ms; ms[6] = whole;
    counts[0] = t.segments; counts[1] = t.longest_segment; counts[2] = t.runs;
    return PIXO_OK;
}

} // extern "C"
