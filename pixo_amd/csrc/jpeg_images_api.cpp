// jpeg_images_api.cpp — JPEG encode of images of individual sizes and colour types anywhere in one block (DESIGN.md §4.3b,
// "Images of individual sizes"): the pixo_hip_jpeg_encode_images* entries, their plan and their driver.
//
// The shared way in (no progressive scans, no optimised tables, no restart markers — the batch entry's condition for one
// pass): the images of a sub-batch go through one ragged coefficient launch per class present (gray or RGB at the template's
// subsampling, times the load form: jpeg_images.hip), then per colour class one coding pass (scan_code<2>: every image a
// byte-aligned segment with its own block count, groups, planes and packed stream) and one stuffing pass (stuff_fused<2>).  The
// number of launches follows the classes present, not the number of images.  Everything else — and a sub-batch whose
// single-pass launch gave up its bounded waits — goes the single way: image after image through encode_file, as
// encode_batch_blocks does.
//
// Sub-batches are greedy in index order, at least one image each, and hold at most pixo_jpeg_images::kSubBatchBlocks = 2^22
// blocks (debug switch jpeg_images_blocks): 512 MiB of tuple at 128 bytes a block, 836 MiB of packed streams at 209.  A
// sub-batch also ends where the way changes, so that each one goes one way as a whole.
//
// The stuffed scans of a sub-batch stay on the device (gray pass: e_out, RGB pass: j_out) until both passes have been sized:
// the files are laid out in index order only then.  Headers differ per image (SOF0 holds the size), so every file is framed
// on the host; scans travel file by file straight into pinned destinations when they are large, and in one copy per pass
// through the context's pinned buffer when they are small (1024 thumbnails: two copies instead of 1024).
// The steps every batch driver takes, and their order: DESIGN.md §4.0; the shared ones: batch_steps.hpp.
#include <algorithm>

#include "batch_steps.hpp"

using namespace pixo_capi;
namespace ji = pixo_jpeg_images;
namespace pd = pixo_dev;

namespace {

struct ImagesPlan {
    struct Image {
        pixo_jpeg_options o; // the template with the image's width, height and colour type written into it
        pixo_host::Geometry g;
        bool shared = false; // the shared way in: ragged launches; otherwise encode_file by itself
    };
    std::vector<Image> image;
    SubBatches sub_first;
};

bool shared_way(const pixo_jpeg_options &o, const pixo_host::Geometry &g)
{
    return !o.progressive && !o.optimize_huffman && !scan_has_restart_markers(o, g) && !debug().host_entropy && !debug().multipass_entropy;
}

void plan_images(const pixo_png_image *images, uint32_t batch, const pixo_jpeg_options &o, ImagesPlan &p)
{
    const uint64_t limit = debug().jpeg_images_blocks ? debug().jpeg_images_blocks : ji::kSubBatchBlocks;
    p.image.resize(batch);
    uint64_t blocks = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        ImagesPlan::Image &x = p.image[i];
        x.o = o;
        x.o.width = images[i].width;
        x.o.height = images[i].height;
        x.o.color_type = images[i].color_type;
        x.g = geometry_of(x.o);
        x.shared = shared_way(x.o, x.g);
        const uint64_t b = x.g.y_blocks + 2 * x.g.c_blocks;
        if (p.sub_first.starts_at(i, blocks + b > limit || (i && x.shared != p.image[i - 1].shared))) blocks = 0; // (also where the way in changes)
        blocks += b;
    }
    p.sub_first.close(batch);
}
int rgb_mode(const pixo_jpeg_options &o) { return o.subsampling == PIXO_S420 ? ji::MODE_420 : ji::MODE_444; }
// The items of a shared sub-batch, in index order; base: the address of the block's first byte
std::vector<ji::Item> items_of(const pixo_png_image *images, uint64_t base, uint32_t first, uint32_t end)
{
    std::vector<ji::Item> items;
    for (uint32_t i = first; i < end; ++i) items.push_back({i - first, base + images[i].offset, images[i].width, images[i].height, images[i].color_type == PIXO_GRAY});
    return items;
}

// Where the files go: blocks of the library's (files) or the caller's arena (offsets; a null arena: sizes only)
struct Sink {
    uint8_t **files = nullptr;
    uint8_t *arena = nullptr;
    size_t cap = 0, at = 0;
    size_t *offsets = nullptr, *lens = nullptr;
    bool pinned = false;
};

// The headers of a colour class, made once: every image's differ in SOF0's height and width only
struct ClassHead {
    std::vector<uint8_t> bytes;
    size_t size_at = 0; // where SOF0's height (2 bytes) and width (2 bytes) lie; 0: not found, make every image's headers
    void make(const pixo_jpeg_options &o)
    {
        bytes.clear();
        pixo_host::file_headers(bytes, o, pixo_host::HuffSet::standard());
        size_at = 0;
        for (size_t i = 2; i + 9 <= bytes.size() && bytes[i] == 0xFF;) { // SOI, then segments: FF, marker, length (2 bytes, itself included)
            if (bytes[i + 1] == 0xC0) { size_at = i + 5; break; }
            i += 2 + ((static_cast<size_t>(bytes[i + 2]) << 8) | bytes[i + 3]);
        }
    }
    void write(uint8_t *dst, const pixo_jpeg_options &o) const
    {
        if (!size_at) {
            std::vector<uint8_t> own;
            pixo_host::file_headers(own, o, pixo_host::HuffSet::standard());
            std::memcpy(dst, own.data(), own.size());
            return;
        }
        std::memcpy(dst, bytes.data(), bytes.size());
        dst[size_at] = static_cast<uint8_t>(o.height >> 8); dst[size_at + 1] = static_cast<uint8_t>(o.height);
        dst[size_at + 2] = static_cast<uint8_t>(o.width >> 8); dst[size_at + 3] = static_cast<uint8_t>(o.width);
    }
};

// One colour class of a shared sub-batch: code<2>, layout, stuff<2> into `out`.  Afterwards `out` holds *scan_bytes bytes, the
// segments back to back, and ends[k] (pinned) says where segment k's end.  kRetryMultipass: a launch gave up its bounded waits.
int code_pass(Context &c, const ji::CodePass &p, const ji::SegRecord *d_records, const int16_t *tuple, Buf &out, unsigned long long *ends, uint64_t *scan_bytes)
{
    pd::ScanArgs a;
    a.y = a.cb = a.cr = tuple; // (the planes come from the records)
    a.tables = c.e_tables.as<uint32_t>();
    a.mode = p.mode == ji::MODE_GRAY ? 0 : (p.mode == ji::MODE_420 ? 2 : 1);
    a.nblocks = p.blocks;
    a.restart = 0;
    a.blocks_per_mcu = p.mode == ji::MODE_GRAY ? 1 : (p.mode == ji::MODE_420 ? 6 : 3);
    a.marker_bytes = 0;
    a.seed_dc[0] = a.seed_dc[1] = a.seed_dc[2] = 0;
    a.bit_base = 0; a.pad_last = 1;
    const size_t stream_cap = static_cast<size_t>(p.stream_words) * 4;
    unsigned long long *base = c.e_segs.as<unsigned long long>();
    pd::SegArgs sg;
    sg.nsegs = p.count;
    sg.groups = p.groups;
    sg.bits = base;
    sg.layout = base + p.count;
    sg.bytes = base + 2 * p.count + 2;
    sg.out_end = base + 3 * p.count + 2;
    sg.host_out_end = ends;
    sg.rag = d_records;
    const size_t code_words = pd::fused_code_state_words_ragged(p.count, p.groups);
    const size_t stuff_words = pd::fused_stuff_state_words(stream_cap) + p.count; // (every segment's last tile is partial)
    const bool zero = c.e_code_state.known >= code_words;
    c.e_code_state.known = 0;
    // (a launch that gives up leaves segments without a length: zero, not what the last call left there, is what the layout
    // and the stuffing kernel then read — no tile of a stream that is not there)
    HIP_TRY(hipMemsetAsync(sg.bits, 0, p.count * 8, c.stream));
    HIP_TRY(pd::launch_scan_code_ragged(a, sg, c.e_code_state.as<unsigned long long>(), zero, c.e_stream.as<uint32_t>(), c.e_stuff_state.as<unsigned long long>(),
                                        stuff_words, mailbox(c), c.stream, debug().spin_budget));
    HIP_TRY(pd::launch_seg_layout(sg, const_cast<unsigned long long *>(sg.layout), const_cast<unsigned long long *>(sg.bytes), mailbox(c), c.stream));
    // tiles: a guess of 64 bytes per block + one partial tile per segment; surplus workgroups leave at once, missing ones are
    // launched below once the layout kernel has said how many there are (scan_stuff_segmented)
    uint64_t first_tile = 0, tiles = pd::stuff_tiles(p.blocks * 64) + p.count;
    size_t want_cap = std::max<size_t>(stream_cap / 4, 4096);
    for (int attempt = 0;; ++attempt) {
        if (const int rc = out.reserve(want_cap)) return rc;
        HIP_TRY(pd::launch_stuff_fused_ragged(c.e_stream.as<uint32_t>(), c.e_code_state.as<unsigned long long>(), code_words, stream_cap + p.count * pd::stuff_tile_bytes(),
                                              first_tile, tiles, c.e_stuff_state.as<unsigned long long>(), /*state_is_zero=*/attempt == 0, out.as<uint8_t>(),
                                              out.cap, mailbox(c), c.stream, sg, debug().spin_budget));
        c.e_code_state.known = code_words;
        HIP_TRY(hipStreamSynchronize(c.stream));
        if (c.mail->totals[3]) return scan_retry_multipass(c);
        const uint64_t all_tiles = c.mail->totals[2];
        if (all_tiles > first_tile + tiles) { // the guess was short: the tiles behind it, same buffers
            if (attempt > 2) return fail(PIXO_ERR_COMPRESSION, "Compression error: packed stream longer than announced");
            first_tile += tiles;
            tiles = all_tiles - first_tile;
            continue;
        }
        *scan_bytes = c.mail->totals[1];
        if (*scan_bytes > out.cap) { // (unusually many 0xFF bytes: grow and repeat the stuffing pass only)
            if (attempt > 2) return fail(PIXO_ERR_COMPRESSION, "Compression error: stuffed stream larger than announced");
            note_route(route::RESTUFF_GROW);
            want_cap = static_cast<size_t>(*scan_bytes);
            first_tile = 0;
            tiles = all_tiles;
            continue;
        }
        return PIXO_OK;
    }
}

// Images [first, end) the shared way.  kRetryMultipass: nothing has been delivered, the caller sends them the single way.
int shared_sub_batch(Context &c, const void *d_px, const pixo_png_image *images, const ImagesPlan &p, uint32_t first, uint32_t end, Sink &sink)
{
    const uint32_t nb = end - first;
    const pixo_jpeg_options &o = p.image[first].o; // (what holds for every image)
    ji::Tables t;
    if (!ji::build_tables(items_of(images, reinterpret_cast<uint64_t>(d_px), first, end), rgb_mode(o), t)) return hip_fail(hipErrorInvalidValue, "tiles of a JPEG images sub-batch");
    // ---- everything reserved before any address goes to a kernel
    int rc;
    const size_t tile_bytes = t.tiles.size() * sizeof(ji::TileRecord), seg_bytes = t.segs.size() * sizeof(ji::SegRecord);
    size_t stream_cap = 0, code_words = 0, stuff_words = 0, most_segs = 0, all_segs = 0;
    for (const ji::CodePass &cp : t.passes) {
        stream_cap = std::max<size_t>(stream_cap, static_cast<size_t>(cp.stream_words) * 4);
        code_words = std::max(code_words, pd::fused_code_state_words_ragged(cp.count, cp.groups));
        stuff_words = std::max(stuff_words, pd::fused_stuff_state_words(static_cast<size_t>(cp.stream_words) * 4) + cp.count);
        most_segs = std::max<size_t>(most_segs, cp.count);
        all_segs += cp.count;
    }
    if ((rc = c.d_coef.reserve(t.blocks * 128)) || (rc = c.h_jtables.reserve(tile_bytes + seg_bytes)) || (rc = c.j_tables.reserve(tile_bytes + seg_bytes)) ||
        (rc = c.e_stream.reserve(stream_cap + 64)) || (rc = c.e_code_state.reserve(code_words * 8)) || (rc = c.e_stuff_state.reserve(stuff_words * 8)) ||
        (rc = c.e_segs.reserve((4 * most_segs + 2) * 8)) || (rc = c.h_segs.reserve(all_segs * 8)) || (rc = c.e_tables.reserve(pixo_scan::kScanTableUpload * 4)))
        return rc;
    const float *qt_all = nullptr;
    if ((rc = device_tables(c.device, &qt_all))) return rc;
    uint32_t packed[pixo_host::kScanTableWords];
    pixo_host::pack_scan_tables(pixo_host::HuffSet::standard(), packed);
    if ((rc = upload_scan_tables(c, packed, c.stream))) return rc;
    std::memcpy(c.h_jtables.p, t.tiles.data(), tile_bytes);
    std::memcpy(c.h_jtables.as<uint8_t>() + tile_bytes, t.segs.data(), seg_bytes);
    HIP_TRY(hipMemcpyAsync(c.j_tables.p, c.h_jtables.p, tile_bytes + seg_bytes, hipMemcpyHostToDevice, c.stream));
    const ji::TileRecord *d_tiles = c.j_tables.as<ji::TileRecord>();
    const ji::SegRecord *d_segs = reinterpret_cast<const ji::SegRecord *>(c.j_tables.as<uint8_t>() + tile_bytes);
    // ---- one coefficient launch per class present
    note_route(route::TWO_KERNEL | route::SEGMENTED_TUPLE | route::SINGLE_PASS_TUPLE);
    for (const ji::CoefLaunch &l : t.launches)
        HIP_TRY(pd::launch_jpeg_images_coeffs(l.mode, l.load, d_tiles + l.first_record, l.count, l.tiles, c.d_coef.as<int16_t>(),
                                              qt_all + (o.quality - 1) * pixo_host::kDeviceQtFloats, c.stream));
    // ---- one coding pass and one stuffing pass per colour class: gray into e_out, RGB into j_out
    std::vector<size_t> scan_at(nb, 0), scan_len(nb, 0); // per image: where its scan lies in its pass's output, how long it is
    std::vector<uint8_t> in_second(nb, 0);
    uint64_t pass_bytes[2] = {0, 0};
    size_t ends_at = 0;
    for (const ji::CodePass &cp : t.passes) {
        const int which = cp.mode == ji::MODE_GRAY ? 0 : 1;
        unsigned long long *ends = c.h_segs.as<unsigned long long>() + ends_at;
        if ((rc = code_pass(c, cp, d_segs + cp.first_record, c.d_coef.as<int16_t>(), which ? c.j_out : c.e_out, ends, &pass_bytes[which]))) return rc;
        for (uint32_t k = 0; k < cp.count; ++k) {
            const uint32_t item = t.seg_item[cp.first_record + k];
            scan_at[item] = k ? static_cast<size_t>(ends[k - 1]) : 0;
            scan_len[item] = static_cast<size_t>(ends[k]) - scan_at[item];
            in_second[item] = static_cast<uint8_t>(which);
        }
        ends_at += cp.count;
    }
    note_route(route::JPEG_IMAGES); // (no pass gave up: this sub-batch's files come from the ragged launches)
    // ---- the files, in index order
    ClassHead head[2];
    for (uint32_t i = 0; i < nb; ++i)
        if (head[in_second[i]].bytes.empty()) head[in_second[i]].make(p.image[first + i].o);
    for (uint32_t i = 0; i < nb; ++i) {
        const size_t len = head[in_second[i]].bytes.size() + scan_len[i] + 2;
        sink.lens[first + i] = len;
        if (sink.offsets) sink.offsets[first + i] = sink.at;
        sink.at += len;
    }
    std::vector<uint8_t *> dst(nb, nullptr);
    bool direct = true; // every destination is pinned: the scans may travel straight into them
    if (sink.files) {
        for (uint32_t i = 0; i < nb; ++i) {
            uint8_t *f = pool_take(sink.lens[first + i]);
            if (!f) { direct = false; f = static_cast<uint8_t *>(std::malloc(sink.lens[first + i])); }
            if (!f) return fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
            sink.files[first + i] = dst[i] = f;
        }
    } else {
        if (!sink.arena || sink.at > sink.cap) return PIXO_OK; // (sizes only: nothing is copied from the sub-batch on that no longer fits)
        for (uint32_t i = 0; i < nb; ++i) dst[i] = sink.arena + sink.offsets[first + i];
        direct = sink.pinned;
    }
    const size_t all_bytes = static_cast<size_t>(pass_bytes[0] + pass_bytes[1]);
    if (direct && all_bytes >= (size_t{4} << 20) * std::max<size_t>(1, nb / 64)) { // (large files: each scan by a copy of its own, no second pass over it)
        note_route(route::JPEG_IMAGES_DIRECT);
        hipError_t e = hipSuccess;
        for (uint32_t i = 0; i < nb && e == hipSuccess; ++i)
            if (scan_len[i])
                e = hipMemcpyAsync(dst[i] + head[in_second[i]].bytes.size(), (in_second[i] ? c.j_out : c.e_out).as<uint8_t>() + scan_at[i], scan_len[i], hipMemcpyDeviceToHost, c.stream);
        const hipError_t idle = hipStreamSynchronize(c.stream); // (also after an error: no copy is in flight when the blocks go back)
        if (e == hipSuccess) e = idle;
        if (e != hipSuccess) return hip_fail(e, "device-to-host copy of the image files");
    } else { // one copy per pass into the context's pinned buffer, from there into the files
        if ((rc = c.h_file.reserve(all_bytes ? all_bytes : 1))) return rc;
        if (pass_bytes[0]) HIP_TRY(hipMemcpyAsync(c.h_file.p, c.e_out.p, pass_bytes[0], hipMemcpyDeviceToHost, c.stream));
        if (pass_bytes[1]) HIP_TRY(hipMemcpyAsync(c.h_file.as<uint8_t>() + pass_bytes[0], c.j_out.p, pass_bytes[1], hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        for (uint32_t i = 0; i < nb; ++i)
            std::memcpy(dst[i] + head[in_second[i]].bytes.size(), c.h_file.as<uint8_t>() + (in_second[i] ? pass_bytes[0] : 0) + scan_at[i], scan_len[i]);
    }
    for (uint32_t i = 0; i < nb; ++i) {
        head[in_second[i]].write(dst[i], p.image[first + i].o);
        const size_t len = sink.lens[first + i];
        dst[i][len - 2] = 0xFF; dst[i][len - 1] = 0xD9;
    }
    return PIXO_OK;
}

// Images [first, end) the single way: each by itself in index order, as encode_batch_blocks / encode_batch_into do
int single_sub_batch(Context &c, const void *d_px, const pixo_png_image *images, const ImagesPlan &p, uint32_t first, uint32_t end, Sink &sink)
{
    for (uint32_t i = first; i < end; ++i) {
        const ImagesPlan::Image &x = p.image[i];
        const FileSource src = FileSource::device(static_cast<const uint8_t *>(d_px) + images[i].offset);
        if (sink.files) {
            if (const int rc = encode_to_block(c, src, x.o, x.g, &sink.files[i], &sink.lens[i])) return rc;
            continue;
        }
        // each straight into its place behind the one before (none once a file did not fit: sizes only)
        const bool room = sink.arena && sink.at < sink.cap;
        uint8_t *dst = room ? sink.arena + sink.at : nullptr;
        const size_t cap = room ? sink.cap - sink.at : 0;
        size_t n = 0;
        FileResult r;
        const int rc = deliver_into(encode_file(c, src, x.o, x.g, FileDest::caller(dst, cap), r), r, dst, cap, &n, /*copy_threads=*/true);
        if (rc && rc != PIXO_ERR_BUFFER_TOO_SMALL) return rc;
        if (rc) sink.cap = 0; // (nothing more is stored)
        sink.offsets[i] = sink.at;
        sink.lens[i] = n;
        sink.at += n;
    }
    return PIXO_OK;
}

int jpeg_images(Context &c, const void *d_px, const pixo_png_image *images, const pixo_jpeg_options &o, uint32_t batch, Sink &sink)
{
    ImagesPlan p;
    plan_images(images, batch, o, p);
    const uint32_t subs = p.sub_first.count();
    if (subs > 1) note_route(route::SUB_BATCHES);
    for (uint32_t part = 0; part < subs; ++part) {
        const uint32_t first = p.sub_first[part], end = p.sub_first[part + 1];
        int rc = kRetryMultipass;
        if (p.image[first].shared) {
            const size_t at = sink.at;
            rc = shared_sub_batch(c, d_px, images, p, first, end, sink);
            if (rc == kRetryMultipass) sink.at = at; // (FALLBACK has been noted: this sub-batch the single way)
        }
        if (rc == kRetryMultipass) rc = single_sub_batch(c, d_px, images, p, first, end, sink);
        if (rc) return rc;
    }
    return PIXO_OK;
}

int images_blocks(Context &c, const void *d_px, const pixo_png_image *images, const pixo_jpeg_options &o, uint32_t batch, uint8_t **files, size_t *lens)
{
    for (uint32_t i = 0; i < batch; ++i) { files[i] = nullptr; lens[i] = 0; }
    Sink sink;
    sink.files = files;
    sink.lens = lens;
    const int rc = jpeg_images(c, d_px, images, o, batch, sink);
    if (rc) {
        (void)hipStreamSynchronize(c.stream); // (no copy is in flight when the blocks go back)
        for (uint32_t i = 0; i < batch; ++i) { free_file(files[i]); files[i] = nullptr; lens[i] = 0; }
    }
    return rc;
}

int images_into(Context &c, const void *d_px, const pixo_png_image *images, const pixo_jpeg_options &o, uint32_t batch, uint8_t *arena, size_t capacity,
                size_t *offsets, size_t *lens)
{
    for (uint32_t i = 0; i < batch; ++i) { offsets[i] = 0; lens[i] = 0; }
    Sink sink;
    sink.arena = arena;
    sink.cap = arena ? capacity : 0;
    sink.offsets = offsets;
    sink.lens = lens;
    const hipMemoryType arena_type = arena ? pointer_info(arena).type : hipMemoryTypeUnregistered;
    // (headers differ per image, and launch_batch_seams writes one header: the files are framed on the host)
    if (arena_type == hipMemoryTypeDevice) return hip_fail(hipErrorInvalidValue, "arena of a JPEG images batch in device memory (host memory only)");
    sink.pinned = arena_type == hipMemoryTypeHost;
    const int rc = jpeg_images(c, d_px, images, o, batch, sink);
    if (rc) return rc;
    return arena && sink.at <= capacity ? PIXO_OK : too_small(sink.at);
}

// The checks the images entries share, in their order (include/pixo_hip.h): those in front of the out-pointers, then (behind
// them) every image's own; *block_end: the furthest image's end.  pixels_name null: the plan entry, which takes no pixels.
int images_checks(const pixo_jpeg_options *options, const void *pixels, const char *pixels_name, const pixo_png_image *images, uint32_t batch)
{
    PIXO_REQUIRE(options);
    pixo_jpeg_options own = *options; // (the template's own fields: its width, height and colour type are not read)
    own.width = own.height = 1;
    own.color_type = PIXO_RGB;
    if (const int rc = checked(own)) return rc;
    if (pixels_name && !pixels) return fail(PIXO_ERR_COMPRESSION, std::string("Compression error: null argument '") + pixels_name + "'");
    PIXO_REQUIRE(images);
    return batch_in_range(batch);
}
int images_check_each(const pixo_jpeg_options &o, const pixo_png_image *images, uint32_t batch, uint64_t *block_end)
{
    *block_end = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        const pixo_png_image &im = images[i];
        pixo_jpeg_options x = o;
        x.width = im.width; x.height = im.height; x.color_type = im.color_type;
        std::string msg;
        int rc = pixo_host::validate(x, false, 0, msg);
        if (rc) return fail(rc, msg + where(i));
        if ((rc = record_extent(im.offset, image_bytes(im), "input", where(i), block_end))) return rc;
    }
    return PIXO_OK;
}

} // namespace

extern "C" {

int pixo_hip_jpeg_encode_images_device(const void *d_pixels, const pixo_png_image *images, uint32_t batch, const pixo_jpeg_options *options,
                                       uint8_t **files, size_t *lens)
{
    uint64_t end = 0;
    int rc = images_checks(options, d_pixels, "d_pixels", images, batch);
    if (rc) return rc;
    PIXO_REQUIRE(files);
    PIXO_REQUIRE(lens);
    if ((rc = images_check_each(*options, images, batch, &end))) return rc;
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return images_blocks(*c, d_pixels, images, *options, batch, files, lens);
}

int pixo_hip_jpeg_encode_images_device_into(const void *d_pixels, const pixo_png_image *images, uint32_t batch, const pixo_jpeg_options *options,
                                            uint8_t *arena, size_t capacity, size_t *offsets, size_t *lens)
{
    CallerStorageScope storage(arena && capacity);
    uint64_t end = 0;
    int rc = images_checks(options, d_pixels, "d_pixels", images, batch);
    if (rc) return rc;
    PIXO_REQUIRE(offsets);
    PIXO_REQUIRE(lens);
    if ((rc = images_check_each(*options, images, batch, &end))) return rc;
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return images_into(*c, d_pixels, images, *options, batch, arena, capacity, offsets, lens);
}

int pixo_hip_jpeg_encode_images(const uint8_t *data, size_t data_len, const pixo_png_image *images, uint32_t batch, const pixo_jpeg_options *options,
                                uint8_t **files, size_t *lens)
{
    uint64_t end = 0;
    int rc = images_checks(options, data, "data", images, batch);
    if (rc) return rc;
    PIXO_REQUIRE(files);
    PIXO_REQUIRE(lens);
    if ((rc = images_check_each(*options, images, batch, &end))) return rc;
    if (data_len < end) return bad_length(static_cast<size_t>(end), data_len);
    PIXO_THREAD_CONTEXT(c);
    if ((rc = upload(c, c.d_px, data, static_cast<size_t>(end)))) return rc;
    return images_blocks(c, c.d_px.p, images, *options, batch, files, lens);
}

int pixo_hip_debug_jpeg_encode_images_plan(const pixo_png_image *images, uint32_t batch, const pixo_jpeg_options *options, uint32_t alignment,
                                           uint32_t *sub_first, uint32_t *sub_count, uint8_t *way_in, uint8_t *load_form, uint64_t *first_group,
                                           uint32_t *coef_launches, uint32_t *entropy_passes)
{
    uint64_t end = 0;
    int rc = images_checks(options, nullptr, nullptr, images, batch);
    if (rc) return rc;
    if (alignment > 15) return fail(PIXO_ERR_COMPRESSION, "Compression error: alignment must be 0..15");
    PIXO_REQUIRE(sub_first);
    PIXO_REQUIRE(sub_count);
    PIXO_REQUIRE(way_in);
    PIXO_REQUIRE(load_form);
    PIXO_REQUIRE(first_group);
    PIXO_REQUIRE(coef_launches);
    PIXO_REQUIRE(entropy_passes);
    if ((rc = images_check_each(*options, images, batch, &end))) return rc;
    ImagesPlan p;
    plan_images(images, batch, *options, p);
    const uint32_t subs = p.sub_first.count();
    p.sub_first.report(sub_first, sub_count);
    *coef_launches = *entropy_passes = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        way_in[i] = p.image[i].shared ? 1 : 0;
        load_form[i] = ji::plan_load_form(ji::load_form_of(alignment + images[i].offset, images[i].width, images[i].color_type == PIXO_GRAY ? 1u : 3u));
        first_group[i] = 0;
    }
    for (uint32_t k = 0; k < subs; ++k) {
        const uint32_t first = p.sub_first[k], last = p.sub_first[k + 1];
        if (!p.image[first].shared) continue;
        ji::Tables t;
        if (!ji::build_tables(items_of(images, alignment, first, last), rgb_mode(*options), t)) return hip_fail(hipErrorInvalidValue, "tiles of a JPEG images sub-batch");
        for (uint32_t i = first; i < last; ++i) first_group[i] = t.first_group[i - first];
        *coef_launches += static_cast<uint32_t>(t.launches.size());
        *entropy_passes += static_cast<uint32_t>(t.passes.size());
    }
    return PIXO_OK;
}

} // extern "C"
