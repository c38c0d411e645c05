// file_route.cpp — pixels or tuple in, a whole file out, to this destination: encode_file, the delivery of its result, and the
// batches built on them.  The entry points (jpeg_api.cpp, bands.cpp) check their arguments, find their context and call these.
#include <algorithm>

#include "capi_internal.hpp"

namespace pixo_capi {

namespace {
// A device tuple on the host, plane by plane (the caller's planes need not be neighbours), in the context's pinned buffer.
int tuple_to_pinned(Context &c, const pixo_host::Geometry &g, const FileSource &t, PlanesOf<const int16_t> &host)
{
    if (const int rc = c.h_coef.reserve((g.y_blocks + 2 * g.c_blocks) * 128)) return rc;
    const Planes h = planes_of(c.h_coef.as<int16_t>(), g);
    HIP_TRY(hipMemcpyAsync(h.y, t.dy, g.y_blocks * 128, hipMemcpyDeviceToHost, c.stream));
    if (g.c_blocks) {
        HIP_TRY(hipMemcpyAsync(h.cb, t.dcb, g.c_blocks * 128, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipMemcpyAsync(h.cr, t.dcr, g.c_blocks * 128, hipMemcpyDeviceToHost, c.stream));
    }
    HIP_TRY(hipStreamSynchronize(c.stream));
    host = {h.y, h.cb, h.cr};
    return PIXO_OK;
}
} // namespace

int encode_file(Context &c, const FileSource &s, const pixo_jpeg_options &o, const pixo_host::Geometry &g, const FileDest &dest, FileResult &r)
{
    int rc;
    const bool twin = debug().host_entropy; // (experiments: the host twin of the entropy stage, baseline and progressive)
    if (twin) note_route(route::HOST_ENTROPY);
    int16_t *dy = nullptr, *dcb = nullptr, *dcr = nullptr;
    if (twin && (s.dy || !o.progressive)) { // host code on a pinned copy of the tuple, tables and all
        PlanesOf<const int16_t> host;
        if (s.host_px) {
            if ((rc = coeffs_to_pinned(c, s.host_px, o, g, &host.y, &host.cb, &host.cr))) return rc;
        } else {
            if (s.d_px && (rc = coeffs_on_device(c, s.d_px, o, g, c.stream, &dy, &dcb, &dcr))) return rc;
            if ((rc = tuple_to_pinned(c, g, s.d_px ? FileSource::tuple(dy, dcb, dcr) : s, host))) return rc;
        }
        pixo_host::encode_file(host.y, host.cb, host.cr, o, r.spill);
        r.file = r.spill.data();
        r.len = r.spill.size();
        return PIXO_OK;
    }
    const size_t px_bytes = pixel_bytes(o, g);
    if (s.host_px && (rc = reserve_pixels(c, px_bytes))) return rc;
    if (o.progressive) {
        if (s.dy) {
            pixo_host::HuffSet h;
            if ((rc = huffman_for_tuple(s.dy, s.dcb, s.dcr, o, g, c, h))) return rc;
            std::vector<uint8_t> head;
            pixo_host::file_headers(head, o, h);
            return device_progressive_scans(s.dy, s.dcb, s.dcr, g, h, c, head, dest, r);
        }
        if (s.host_px) HIP_TRY(hipMemcpyAsync(c.d_px.p, s.host_px, px_bytes, hipMemcpyHostToDevice, c.stream));
        return progressive_to_view(s.host_px ? c.d_px.p : s.d_px, o, g, c, twin, dest, r);
    }
    if (s.dy) return encode_baseline_file(c, s.dy, s.dcb, s.dcr, nullptr, o, g, dest, r);
    // Device pixels into a block of the library's: the coefficient kernel, then the tuple's route.  Host pixels, and device pixels
    // into caller storage: the entropy stage gets the pixels and launches the uploads and the coefficient kernel itself — whole, band
    // by band while the file's first pieces travel back (pieces.cpp), or not at all (the fused pixel -> scan kernel).
    if (s.d_px && dest.kind == DestKind::OwnBlock) {
        if ((rc = coeffs_on_device(c, s.d_px, o, g, c.stream, &dy, &dcb, &dcr))) return rc;
        return encode_baseline_file(c, dy, dcb, dcr, nullptr, o, g, dest, r);
    }
    if ((rc = coeffs_reserve(c, g, &dy, &dcb, &dcr))) return rc;
    const PixelSource src{s.host_px ? c.d_px.p : s.d_px, &o, &g, dy, dcb, dcr, s.host_px};
    return encode_baseline_file(c, dy, dcb, dcr, &src, o, g, dest, r);
}

int deliver_block(FileResult &r, uint8_t **out, size_t *out_len)
{
    if (r.own_block) { // (the device-to-host copy went straight into the block the caller gets)
        *out = const_cast<uint8_t *>(r.file);
        *out_len = r.len;
        return PIXO_OK;
    }
    Stopwatch sw;
    const int rc = deliver(r.file, r.len, out, out_len);
    sw.lap("file into fresh host memory");
    return rc;
}

int deliver_into(int rc, const FileResult &r, uint8_t *output, size_t capacity, size_t *out_len, bool copy_threads)
{
    if (rc == PIXO_OK || rc == PIXO_ERR_BUFFER_TOO_SMALL) *out_len = r.len; // (the size needed when the file does not fit)
    if (rc || r.file == output) return rc; // (in place: copied or stored from the device straight into the caller's storage)
    if (!output || r.len > capacity) return too_small(r.len);
    if (copy_threads) big_copy(output, r.file, r.len);
    else std::memcpy(output, r.file, r.len);
    return PIXO_OK;
}

int encode_to_block(Context &c, const FileSource &src, const pixo_jpeg_options &o, const pixo_host::Geometry &g, uint8_t **out, size_t *out_len)
{
    FileResult r;
    const int rc = encode_file(c, src, o, g, FileDest::own_block(), r);
    return rc ? rc : deliver_block(r, out, out_len);
}

int encode_host_pixels(const uint8_t *data, const pixo_jpeg_options &o, const FileDest &dest, FileResult &r)
{
    Context &c = thread_context();
    if (const int rc = c.ensure()) return rc;
    PIXO_ON_DEVICE_OF(c);
    return encode_file(c, FileSource::host(data), o, geometry_of(o), dest, r);
}

// ---- batches ---------------------------------------------------------------------------------------------------------------
namespace {
// The entropy-coded bytes of a batch in c.e_out: one coefficient launch + one pass of the entropy stage (the images are
// segments of the single-pass kernels).  Only for option sets that allow it (batch_in_one_pass).
int batch_on_device(Context &c, const void *d_pixels, const pixo_jpeg_options &o, const pixo_host::Geometry &g, uint32_t batch,
                    std::vector<uint8_t> &head, std::vector<uint64_t> &starts, bool *gaps)
{ // *gaps: the scans lie in c.e_out with room for EOI + the next file's headers between them (the files' final spacing)
    std::vector<uint8_t> probe_head;
    pixo_host::file_headers(probe_head, o, pixo_host::HuffSet::standard()); // (a one-pass batch has the standard tables)
    const uint32_t gap = static_cast<uint32_t>(probe_head.size() + 2);
    const float *qt_all = nullptr;
    int rc = device_tables(c.device, &qt_all);
    if (rc) return rc;
    if ((rc = c.d_coef.reserve((g.y_blocks + 2 * g.c_blocks) * 128 * batch))) return rc;
    const Planes t = planes_of(c.d_coef.as<int16_t>(), g, batch);
    // (the entropy stage gets the PIXELS — an RGB batch goes through the fused pixel -> scan kernel, every image a segment,
    // and never writes the tuple; otherwise the stage launches the coefficient kernel over the batch itself)
    const PixelSource src{d_pixels, &o, &g, t.y, t.cb, t.cr};
    FileResult r;
    if ((rc = encode_baseline_file(c, t.y, t.cb, t.cr, &src, o, g, FileDest::in_hbm(batch, gap), r))) return rc;
    head = std::move(r.head);
    starts = std::move(r.image_starts);
    *gaps = r.gaps_left;
    return PIXO_OK;
}
bool batch_in_one_pass(const pixo_jpeg_options &o, const pixo_host::Geometry &g, uint32_t batch)
{
    return batch > 1 && !o.progressive && !o.optimize_huffman && !scan_has_restart_markers(o, g) && pixel_bytes(o, g) % 4 == 0;
}
const void *image_at(const void *d_pixels, size_t px_bytes, uint32_t i) { return static_cast<const uint8_t *>(d_pixels) + i * px_bytes; }
// Image i of a one-pass batch: hdr header bytes, its scan, EOI.  gap: what the batch left free between two scans in c.e_out.
size_t batch_file_len(const std::vector<uint64_t> &starts, uint32_t i, uint32_t batch, size_t hdr, size_t gap)
{
    return hdr + static_cast<size_t>(starts[i + 1] - starts[i]) - (i + 1 < batch ? gap : 0) + 2;
}
// Headers in front of a scan that lies at its place in a file of `len` bytes, EOI behind it.
void frame_file(uint8_t *p, const std::vector<uint8_t> &head, size_t len)
{
    std::memcpy(p, head.data(), head.size());
    p[len - 2] = 0xFF; p[len - 1] = 0xD9;
}
} // namespace

int encode_batch_blocks(Context &c, const void *d_pixels, const pixo_jpeg_options &o, const pixo_host::Geometry &g, uint32_t batch,
                        uint8_t **files, size_t *lens)
{
    int rc = PIXO_OK;
    for (uint32_t i = 0; i < batch; ++i) { files[i] = nullptr; lens[i] = 0; }
    auto release = [&](int code) { for (uint32_t i = 0; i < batch; ++i) { free_file(files[i]); files[i] = nullptr; } return code; };
    if (!batch_in_one_pass(o, g, batch)) { // per-image tables or segments inside the images: one image at a time
        for (uint32_t i = 0; i < batch; ++i)
            if ((rc = encode_to_block(c, FileSource::device(image_at(d_pixels, pixel_bytes(o, g), i)), o, g, &files[i], &lens[i]))) return release(rc);
        return PIXO_OK;
    }
    std::vector<uint8_t> head;
    std::vector<uint64_t> starts;
    bool gaps = false;
    if ((rc = batch_on_device(c, d_pixels, o, g, batch, head, starts, &gaps))) return rc;
    const size_t hdr = head.size(), scan_bytes = static_cast<size_t>(starts[batch]);
    for (uint32_t i = 0; i < batch; ++i) lens[i] = batch_file_len(starts, i, batch, hdr, gaps ? hdr + 2 : 0);
    // Every file's block comes from the library's pool of PINNED host memory (host_memory.cpp pool_take) and its entropy-coded bytes are
    // copied from the device straight into it — 64 x 1080p noise: 26.8 -> ~2.5 ms a batch, where fresh malloc'd blocks cost 22,000 page
    // faults.  The pool exhausted (or debug switch plain_host): once over PCIe into the context's pinned buffer (a copy into fresh pageable
    // blocks would make the runtime pin new pages every call), from there into malloc'd files by several threads (page-fault bound).
    bool pooled = true;
    for (uint32_t i = 0; i < batch && pooled; ++i)
        if (!(files[i] = pool_take(lens[i]))) pooled = false;
    hipError_t e = hipSuccess;
    if (pooled) {
        for (uint32_t i = 0; i < batch && e == hipSuccess; ++i) {
            const size_t seg = lens[i] - hdr - 2;
            if (seg) e = hipMemcpyAsync(files[i] + hdr, c.e_out.as<uint8_t>() + starts[i], seg, hipMemcpyDeviceToHost, c.stream);
        }
        for (uint32_t i = 0; i < batch; ++i) frame_file(files[i], head, lens[i]); // (while the copies run: they touch other bytes)
    } else {
        (void)release(0);
        if ((rc = c.h_file.reserve(scan_bytes ? scan_bytes : 1))) return rc;
        e = hipMemcpyAsync(c.h_file.p, c.e_out.p, scan_bytes, hipMemcpyDeviceToHost, c.stream);
        for (uint32_t i = 0; i < batch && !rc; ++i)
            if (!(files[i] = static_cast<uint8_t *>(std::malloc(lens[i])))) rc = fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
    }
    // The one exit of both: the stream is idle before any block goes back to the pool or to free — a copy enqueued before a
    // failure may still be writing into them.
    const hipError_t idle = hipStreamSynchronize(c.stream);
    if (e == hipSuccess) e = idle;
    if (!rc && e != hipSuccess) rc = hip_fail(e, "device-to-host copy of the batch files");
    if (rc) return release(rc);
    if (pooled) return PIXO_OK;
    const size_t total = scan_bytes + static_cast<size_t>(batch) * (hdr + 2);
    const unsigned t = std::max(1u, static_cast<unsigned>(std::min<size_t>(std::min<size_t>(debug().copy_threads, batch), total >> 21)));
    run_on_threads(t, [&](unsigned k) {
        for (uint32_t i = k; i < batch; i += t) {
            frame_file(files[i], head, lens[i]);
            std::memcpy(files[i] + hdr, c.h_file.as<uint8_t>() + starts[i], lens[i] - hdr - 2);
        }
    });
    return PIXO_OK;
}

namespace {
struct Arena {
    uint8_t *p;
    size_t cap;
    bool pinned, device; // (neither: pageable host memory, or none at all)
};

// Into how many sub-batches a one-pass batch is cut.  Only where the files are large enough for their copy to matter: smooth
// content (0.6 bytes per block) is 3.6 MB for 64 x 1080p, and eight passes cost 0.66 ms where one takes 0.43; in between
// (photograph-like content, 3-8 bytes per block: 22 MB) four sub-batches — 0.76 -> 0.61 ms, where eight take 0.73
// (profiles/r05_batch_parts.txt).  one_plus_per_block: the context's memory of the last batch (0: none).
uint32_t sub_batch_parts(size_t batch_px_bytes, uint32_t batch, uint32_t one_plus_per_block)
{
    constexpr uint32_t kWorthIt = 8, kMedium = 3; // bytes per block
    if (batch_px_bytes < (size_t{64} << 20)) return 1;
    if (one_plus_per_block == 0 || one_plus_per_block > kWorthIt) return std::min<uint32_t>(std::max<uint32_t>(batch / 8, 1), 8);
    if (one_plus_per_block > kMedium) return std::min<uint32_t>(std::max<uint32_t>(batch / 16, 1), 4);
    return 1;
}

// A one-pass batch's scans into their places in the arena; *total: the bytes of all files (nothing is copied from the sub-batch
// on that no longer fits).  The files' headers and EOI are the caller's.
// Sub-batches alternate between two contexts (two streams, two sets of buffers): the device-to-host copy of one
// sub-batch's files runs while the next one's kernels do — 64 x 1080p noise: 88.9 MB over PCIe are 1.7 ms, the kernels
// of the whole batch 0.4 ms; in one pass they added up (2.08 ms).  A sub-batch's place in the arena is known when the
// one before has been sized (its entropy pass ends with that read-back), before its bytes have moved.
// The context remembers the last batch's bytes per block; an unknown or changed content is found out after the first
// sub-batch, the rest then goes in one pass.
int batch_scans_into_arena(Context &c, const void *d_pixels, const pixo_jpeg_options &o, const pixo_host::Geometry &g, uint32_t batch,
                           const Arena &arena, size_t *offsets, size_t *lens, std::vector<uint8_t> &head, size_t *total)
{
    const size_t px_bytes = pixel_bytes(o, g), blocks_per_image = g.y_blocks + 2 * g.c_blocks;
    uint32_t parts = sub_batch_parts(px_bytes * batch, batch, c.batch_per_block);
    if (debug().batch_parts) parts = debug().batch_parts;
    // (every sub-batch holds two images or more: a sub-batch of one would take the single-image path, whose files are not
    // left in the context's buffer at their batch spacing — no image starts to place them by)
    parts = std::max<uint32_t>(std::min<uint32_t>(parts, batch / 2), 1);
    Context *second = nullptr;
    if (parts > 1) {
        note_route(route::SUB_BATCHES);
        second = pool().take(c.device);
        if (second && (second->ensure() || order_after_producer(*second))) { pool().give(second); second = nullptr; }
    }
    size_t at = 0;
    uint32_t first = 0;
    int rc = PIXO_OK;
    if (arena.p && !arena.pinned && !arena.device) advise_huge(arena.p, arena.cap);
    for (uint32_t part = 0; part < parts && !rc; ++part) {
        uint32_t nb = (batch - first + (parts - part) - 1) / (parts - part);
        Context &cx = (second && (part & 1)) ? *second : c;
        std::vector<uint64_t> starts;
        bool gaps = false;
        if ((rc = batch_on_device(cx, image_at(d_pixels, px_bytes, first), o, g, nb, head, starts, &gaps))) break;
        if (starts.size() < static_cast<size_t>(nb) + 1) { // (the layout below needs where every image's bytes begin)
            rc = fail(PIXO_ERR_COMPRESSION, "Compression error: sub-batch of " + std::to_string(nb) + " image(s) without image starts");
            break;
        }
        const size_t hdr = head.size(), at0 = at, run = static_cast<size_t>(starts[nb]);
        for (uint32_t i = 0; i < nb; ++i) {
            offsets[first + i] = at;
            lens[first + i] = batch_file_len(starts, i, nb, hdr, gaps ? hdr + 2 : 0);
            at += lens[first + i];
        }
        if (at <= arena.cap) {
            hipError_t e = hipSuccess;
            if (gaps && !arena.pinned && !arena.device) { // pageable arena: through the context's pinned buffer + the copy threads (a copy
                                                          // straight into pageable pages makes the runtime fault them in and pin them as it goes)
                if (run) {
                    if ((rc = cx.h_file.reserve(run))) break;
                    e = hipMemcpyAsync(cx.h_file.p, cx.e_out.p, run, hipMemcpyDeviceToHost, cx.stream);
                    if (e == hipSuccess) e = hipStreamSynchronize(cx.stream);
                    if (e == hipSuccess) big_copy(arena.p + at0 + hdr, cx.h_file.as<uint8_t>(), run);
                }
            } else if (gaps) { // the scans lie in the device buffer at their files' final spacing: ONE copy, the gaps are filled in afterwards
                               // (device arena: the files stay in HBM for a caller that gathers them over RCCL, pixo_amd/sharded.py)
                if (run) e = hipMemcpyAsync(arena.p + at0 + hdr, cx.e_out.p, run, arena.device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, cx.stream);
            } else { // (multi-pass kernels: every file's entropy-coded bytes by a copy of its own)
                for (uint32_t i = 0; i < nb && e == hipSuccess; ++i) {
                    const size_t seg = lens[first + i] - hdr - 2;
                    if (seg) e = hipMemcpyAsync(arena.p + offsets[first + i] + hdr, cx.e_out.as<uint8_t>() + starts[i], seg,
                                                arena.device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, cx.stream);
                }
            }
            if (e != hipSuccess) rc = hip_fail(e, "device-to-host copy of the batch");
        }
        first += nb;
        const size_t per_block = (at - at0) / (static_cast<size_t>(nb) * blocks_per_image);
        c.batch_per_block = static_cast<uint32_t>(1 + per_block);
        if (part == 0 && parts > 1 && !debug().batch_parts) { // (what the content really is: the rest in as many passes as that is worth)
            const uint32_t want = sub_batch_parts(px_bytes * batch, batch, c.batch_per_block);
            if (want < parts) parts = std::max<uint32_t>(want, 2);
        } // (small files after all: everything else in one more pass)
    }
    // (both streams: also after an error, the second context goes back to the pool idle)
    hipError_t e = hipStreamSynchronize(c.stream);
    if (second) {
        const hipError_t e2 = hipStreamSynchronize(second->stream);
        if (e == hipSuccess) e = e2;
        pool().give(second);
    }
    if (!rc && e != hipSuccess) rc = hip_fail(e, "device-to-host copy of the batch");
    *total = at;
    return rc;
}
} // namespace

int encode_batch_into(Context &c, const void *d_pixels, const pixo_jpeg_options &o, const pixo_host::Geometry &g, uint32_t batch,
                      uint8_t *arena_p, size_t capacity, size_t *offsets, size_t *lens)
{
    int rc = PIXO_OK;
    const size_t px_bytes = pixel_bytes(o, g);
    for (uint32_t i = 0; i < batch; ++i) { offsets[i] = 0; lens[i] = 0; }
    const hipMemoryType arena_type = arena_p ? pointer_info(arena_p).type : hipMemoryTypeUnregistered;
    const Arena arena{arena_p, capacity, arena_type == hipMemoryTypeHost, arena_type == hipMemoryTypeDevice};
    size_t at = 0;
    if (!batch_in_one_pass(o, g, batch)) { // per-image tables / segments inside the images: one image at a time
        bool fits = true;
        hipError_t e = hipSuccess;
        for (uint32_t i = 0; i < batch && e == hipSuccess; ++i) {
            const FileSource src = FileSource::device(image_at(d_pixels, px_bytes, i));
            size_t n = 0;
            if (arena.device) { // files to stay in HBM: each image through a host file, then host-to-device behind the one before
                uint8_t *f = nullptr;
                if ((rc = encode_to_block(c, src, o, g, &f, &n))) return rc;
                if (at + n <= capacity) e = hipMemcpy(arena.p + at, f, n, hipMemcpyHostToDevice);
                free_file(f);
            } else { // each straight into its place behind the one before (none once a file did not fit: sizes only)
                uint8_t *dst = fits && arena.p && at < capacity ? arena.p + at : nullptr;
                FileResult r;
                rc = deliver_into(encode_file(c, src, o, g, FileDest::caller(dst, capacity - at), r), r, dst, capacity - at, &n, /*copy_threads=*/true);
                if (rc == PIXO_ERR_BUFFER_TOO_SMALL) fits = false;
                else if (rc) return rc;
            }
            offsets[i] = at; lens[i] = n;
            at += n;
        }
        if (e != hipSuccess) return hip_fail(e, "host-to-device copy of a batch file");
        return fits && at <= capacity ? PIXO_OK : too_small(at);
    }
    std::vector<uint8_t> head;
    if ((rc = batch_scans_into_arena(c, d_pixels, o, g, batch, arena, offsets, lens, head, &at))) return rc;
    if (at > capacity) return too_small(at);
    const size_t hdr = head.size();
    if (arena.device) { // headers and EOI markers: one small upload (offsets + the header bytes) and one launch, a workgroup per seam
        std::vector<uint64_t> meta(batch + 1 + (hdr + 7) / 8);
        for (uint32_t i = 0; i < batch; ++i) meta[i] = offsets[i];
        meta[batch] = at;
        std::memcpy(meta.data() + batch + 1, head.data(), hdr);
        if ((rc = c.e_seams.reserve(meta.size() * 8))) return rc;
        hipError_t e = hipMemcpyAsync(c.e_seams.p, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, c.stream);
        if (e == hipSuccess) e = pixo_dev::launch_batch_seams(arena.p, c.e_seams.as<unsigned long long>(), batch, static_cast<uint32_t>(hdr), c.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
        return e == hipSuccess ? PIXO_OK : hip_fail(e, "headers of the batch files");
    }
    for (uint32_t i = 0; i < batch; ++i) frame_file(arena.p + offsets[i], head, lens[i]);
    return PIXO_OK;
}

} // namespace pixo_capi
