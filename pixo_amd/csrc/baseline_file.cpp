// baseline_file.cpp — whole baseline files from a device tuple, or from pixels not transformed yet: the route baseline_plan.hpp
// chooses, run; every route ends in finish_file.
#include <algorithm>

#include "capi_internal.hpp"

namespace pixo_capi {
namespace {

using Form = BaselinePlan::Form;
using Direct = BaselinePlan::Direct;
using Upload = BaselinePlan::Upload;

PlanFacts plan_facts(const Context &c, const ScanJob &j, const pixo_jpeg_options &o, const pixo_host::Geometry &g, const PixelSource *src,
                     const FileDest &d, bool dest_gpu_writable)
{
    const DebugSwitches &s = debug();
    PlanFacts f;
    f.blocks = j.n;
    f.fused = j.fused;
    f.segmented = j.segmented;
    f.batch = d.batch;
    f.pixels = src != nullptr;
    f.host_pixels = src && src->host_px;
    f.pixel_bytes = pixel_bytes(o, g);
    f.pixels_code_usable = src && pixels_code_usable(j, o, g, d.batch);
    f.optimize_huffman = o.optimize_huffman;
    f.dest = d.kind;
    f.dest_cap = d.cap;
    f.dest_gpu_writable = dest_gpu_writable;
    f.last_scan_bytes = c.last_scan_bytes;
    f.last_scan_blocks = c.last_scan_blocks;
    f.one_piece = s.one_piece;
    f.direct_stores = s.direct_stores;
    f.no_direct_small = s.no_direct_small;
    f.fused_batch = s.fused_batch;
    f.no_bands_upload = s.no_bands_upload;
    f.bands_upload_min_mb = s.bands_upload_min_mb;
    f.piece_groups = s.piece_groups;
    f.piece_medium = s.piece_medium;
    f.piece_medium_forced = s.piece_medium_forced;
    return f;
}

// The context's history, which the next file's plan goes by (whole single images only).
void remember_scan(Context &c, uint64_t bytes, uint64_t blocks)
{
    if (!blocks) return;
    c.last_scan_bytes = bytes;
    c.last_scan_blocks = blocks;
}

// Where every image of a batch begins in the stuffed scans (batch + 1 entries).  A copy may still be on its way: the stream is
// synchronised before they are read.
int batch_image_starts(Context &c, const ScanJob &j, uint32_t batch, uint64_t scan_bytes, std::vector<uint64_t> &starts)
{
    starts.assign(batch + 1, 0);
    if (j.segmented || j.pc_seg) { // the stuffing kernel / the fused kernel left every image's end in the pinned mailbox
        // (h_segs[i]: where image i's bytes end; the next image begins behind the gap)
        const uint64_t *ends = c.h_segs.as<uint64_t>();
        for (uint32_t i = 0; i < batch; ++i) starts[i + 1] = ends[i] + (i + 1 < batch ? j.seg.marker_bytes : 0);
        return PIXO_OK;
    }
    // where every image's segment begins in the stuffed stream (reuses the seg_bytes buffer: 8 B/entry)
    if (const int rc = c.e_seg_bytes.reserve(j.nseg * 8)) return rc;
    HIP_TRY(pixo_dev::launch_segment_out_offsets(j.plan, j.nbytes, c.e_stream.as<uint32_t>(), c.e_tile_base.as<uint64_t>(),
                                                 c.e_seg_bytes.as<uint64_t>(), c.stream));
    HIP_TRY(hipMemcpyAsync(starts.data(), c.e_seg_bytes.p, j.nseg * 8, hipMemcpyDeviceToHost, c.stream));
    starts[batch] = scan_bytes;
    return PIXO_OK;
}

// Every route ends here.  The scan's bytes lie at placed + head.size() (pieces, direct stores: stored in place) or in c.e_out;
// the headers are written once, here, and EOI behind the scan (not for scans left in HBM: the caller delivers them).
int finish_file(Context &c, const FileDest &d, const ScanJob &j, const std::vector<uint8_t> &head, uint64_t scan_bytes, uint8_t *placed,
                FileResult &r)
{
    const size_t hdr = head.size(), total = hdr + scan_bytes + 2;
    const bool fits = d.kind != DestKind::Caller || total <= d.cap;
    if (placed && !fits) return too_small(total, &r.len); // (stored in place up to the storage's end: nothing to remember)
    if (d.batch == 1) remember_scan(c, scan_bytes, j.n);
    else if (const int rc = batch_image_starts(c, j, d.batch, scan_bytes, r.image_starts)) return rc;
    if (d.kind == DestKind::InHbm) {
        if (!j.segmented && !j.pc_seg) HIP_TRY(hipStreamSynchronize(c.stream)); // (image_starts is being copied)
        r.head = head;
        r.file = nullptr;
        r.len = static_cast<size_t>(scan_bytes);
        r.header_len = hdr;
        return PIXO_OK;
    }
    if (!fits) return too_small(total, &r.len);
    uint8_t *buf = placed;
    if (!buf) { // copied out of c.e_out: into the caller's storage, a block the caller will own, or the pinned buffer
        bool mine = false;
        if (d.kind == DestKind::Caller) {
            buf = d.p;
        } else if (d.kind == DestKind::OwnBlock) {
            if (!(buf = alloc_file(total))) return fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
            mine = true;
        } else {
            if (const int rc = c.h_file.reserve(total)) return rc;
            buf = c.h_file.as<uint8_t>();
        }
        hipError_t ce = hipMemcpyAsync(buf + hdr, c.e_out.p, scan_bytes, hipMemcpyDeviceToHost, c.stream);
        if (ce == hipSuccess) ce = hipStreamSynchronize(c.stream);
        if (ce != hipSuccess) {
            if (mine) std::free(buf);
            return hip_fail(ce, "device-to-host copy of the file");
        }
        r.own_block = mine;
    }
    std::memcpy(buf, head.data(), hdr);
    buf[hdr + scan_bytes] = 0xFF; // EOI
    buf[hdr + scan_bytes + 1] = 0xD9;
    r.file = buf;
    r.len = total;
    r.header_len = hdr;
    return PIXO_OK;
}

int upload_pixels(Context &c, const PixelSource &src, const pixo_jpeg_options &o, const pixo_host::Geometry &g)
{
    HIP_TRY(hipMemcpyAsync(const_cast<void *>(src.d_px), src.host_px, pixel_bytes(o, g), hipMemcpyHostToDevice, c.stream));
    return PIXO_OK;
}

// The tuple of the whole image — of a batch: every plane of all images back to back, src.dy / dcb / dcr point into that layout.
int coeffs_whole(Context &c, const PixelSource &src, const pixo_jpeg_options &o, const pixo_host::Geometry &g, uint32_t batch)
{
    if (batch == 1) return coeffs_rows(c, src.d_px, o, g, c.stream, src.dy, src.dcb, src.dcr, 0, 0);
    const float *qt_all = nullptr;
    if (const int rc = device_tables(c.device, &qt_all)) return rc;
    HIP_TRY(pixo_dev::launch_jpeg_coeffs(src.d_px, o.width, o.height, g.gray, g.s420, batch, src.dy, g.gray ? nullptr : src.dcb,
                                         g.gray ? nullptr : src.dcr, qt_all + (o.quality - 1) * pixo_host::kDeviceQtFloats, c.stream));
    return PIXO_OK;
}

// A scan in pieces, into the caller's storage (the plan made sure it holds any file the pieces are sized for) or the context's
// pinned buffer.  1: the scan outgrew the pieces' guesses and nothing of it is kept.
int run_pieces(Context &c, ScanJob &j, const PixelSource *src, const pixo_jpeg_options &o, const pixo_host::Geometry &g,
               const BaselinePlan &p, const FileDest &d, FileResult &r)
{
    Stopwatch sw;
    int rc = PIXO_OK;
    PixelSource device_src; // (the same source once the pixels are on the device)
    if (p.upload == Upload::OneCopy && (rc = upload_pixels(c, *src, o, g))) return rc;
    if (p.coeffs_first) {
        if ((rc = coeffs_whole(c, *src, o, g, 1))) return rc;
        src = nullptr;
    } else if (p.upload == Upload::OneCopy) {
        device_src = *src;
        device_src.host_px = nullptr;
        src = &device_src;
    }
    if ((rc = scan_tables(c, j, o, g, c.stream, nullptr))) return rc;
    std::vector<uint8_t> head;
    pixo_host::file_headers(head, o, j.h);
    const size_t hdr = head.size(), bound = pieces_file_bound(j.n);
    uint8_t *buf = d.p;
    size_t cap = d.cap;
    if (d.kind == DestKind::Caller) {
        advise_huge(buf, std::min(cap, bound));
    } else {
        if ((rc = c.h_file.reserve(bound))) return rc;
        buf = c.h_file.as<uint8_t>();
        cap = c.h_file.cap;
    }
    uint64_t scan_bytes = 0;
    rc = device_entropy_pieces(c, j, c.stream, buf + hdr, cap - hdr - 2, &scan_bytes, src);
    r.tuple_done = true; // (whatever happened)
    sw.lap("code+stuff+copy (pieces)");
    if (rc) return rc;
    return finish_file(c, d, j, head, scan_bytes, buf, r);
}

// One piece: the fused pixel -> scan kernel, or the tuple coders behind the coefficient kernel.  The stuffing kernel stores
// straight into host memory where the plan says so (and caller storage holds more than the headers), otherwise into c.e_out.
int run_one_piece(Context &c, ScanJob &j, const PixelSource *src, const pixo_jpeg_options &o, const pixo_host::Geometry &g,
                  const BaselinePlan &p, const FileDest &d, uint8_t *dest_dev, FileResult &r)
{
    Stopwatch sw;
    int rc = PIXO_OK;
    if (p.upload == Upload::OneCopy && (rc = upload_pixels(c, *src, o, g))) return rc;
    if (p.coeffs_first && (rc = coeffs_whole(c, *src, o, g, d.batch))) return rc;
    if (p.form != Form::Pixels) r.tuple_done = true;
    std::vector<uint8_t> head;
    if (p.form == Form::MultiPass) {
        if ((rc = scan_lengths(c, j, o, g, c.stream, nullptr))) return rc;
        if ((rc = scan_pack(c, j, c.stream))) return rc;
        sw.lap("lengths+pack (multi-pass)");
        pixo_host::file_headers(head, o, j.h);
        return finish_file(c, d, j, head, j.scan_bytes, nullptr, r);
    }
    const bool pixels = p.form == Form::Pixels;
    if (pixels && o.optimize_huffman) j.count_px = src->d_px; // (optimised tables: the statistics from the pixels as well — scan_tables)
    if ((rc = pixels ? scan_tables(c, j, o, g, c.stream, nullptr) : scan_lengths(c, j, o, g, c.stream, nullptr, /*wait=*/false))) return rc;
    pixo_host::file_headers(head, o, j.h); // (the tables are known now)
    HostTarget target;
    bool direct = false;
    if (p.direct == Direct::PinnedBuffer) {
        target.grow = true;
        target.before = head.size();
        target.after = 2;
        direct = true;
    } else if (p.direct == Direct::CallerStorage && d.cap > head.size() + 2) {
        target.p = dest_dev + head.size();
        target.cap = d.cap - head.size() - 2;
        direct = true;
    }
    if (direct && !pixels) note_route(route::DIRECT_STORES);
    if (pixels) rc = scan_from_pixels(c, j, o, g, c.stream, src->d_px, direct ? &target : nullptr, /*wait=*/true, d.batch);
    else rc = scan_stuff_fused(c, j, c.stream, 0, nullptr, nullptr, nullptr, /*chained=*/true, direct ? &target : nullptr);
    if (rc) return rc;
    sw.lap("code+stuff (fused)");
    uint8_t *placed = !direct ? nullptr : d.kind == DestKind::Caller ? d.p : c.h_file.as<uint8_t>(); // (h_file only now: the kernel may have grown it)
    return finish_file(c, d, j, head, j.scan_bytes, placed, r);
}

// One attempt at the file: plan, run the plan.  A pieces attempt that starts over is planned again from the tuple, in one piece.
int encode_once(Context &c, const int16_t *dy, const int16_t *dcb, const int16_t *dcr, const PixelSource *src, const pixo_jpeg_options &o,
                const pixo_host::Geometry &g, const FileDest &d, uint8_t *dest_dev, FileResult &r)
{
    if (!src) r.tuple_done = true;
    ScanJob j;
    j.seg_gap = d.batch > 1 ? d.seg_gap : 0;
    if (const int rc = scan_begin(c, j, dy, dcb, dcr, o, g, d.batch, nullptr)) return rc;
    const PlanFacts facts = plan_facts(c, j, o, g, src, d, dest_dev != nullptr);
    BaselinePlan p = plan_baseline_file(facts);
    note_route(p.notes);
    // (the fused kernel leaves any gap between its segments; the single-pass tuple coders the gaps scan_begin accepted)
    r.gaps_left = d.seg_gap != 0 && (p.form == Form::Pixels && d.batch > 1 ? j.seg_gap == d.seg_gap : j.segmented && j.seg.marker_bytes == d.seg_gap);
    if (p.form == Form::Pieces) {
        const int rc = run_pieces(c, j, src, o, g, p, d, r);
        if (rc != 1) return rc;
        c.e_code_state.known = 0; // (the pieces' kernels left it dirty)
        note_route(route::PIECES_REDO);
        p = plan_baseline_file(tuple_computed_no_pieces(facts));
        note_route(p.notes);
        src = nullptr;
    }
    return run_one_piece(c, j, src, o, g, p, d, dest_dev, r);
}

} // namespace

int encode_baseline_file(Context &c, const int16_t *dy, const int16_t *dcb, const int16_t *dcr, const PixelSource *src,
                         const pixo_jpeg_options &o, const pixo_host::Geometry &g, const FileDest &d, FileResult &r)
{
    uint8_t *dest_dev = nullptr; // caller storage the GPU can store into (pinned / registered): its device address
    if (d.kind == DestKind::Caller && d.cap) {
        const PointerInfo at = pointer_info(d.p);
        if (at.type == hipMemoryTypeHost) dest_dev = static_cast<uint8_t *>(at.device_ptr);
    }
    int rc = encode_once(c, dy, dcb, dcr, src, o, g, d, dest_dev, r);
    if (rc != kRetryMultipass) return rc;
    // a single-pass kernel gave up waiting (its waits are bounded): the same scan with the multi-pass kernels, from the tuple if
    // the first attempt computed it
    RetryMultipass scope;
    rc = encode_once(c, dy, dcb, dcr, r.tuple_done ? nullptr : src, o, g, d, dest_dev, r);
    return rc == kRetryMultipass ? fail(PIXO_ERR_COMPRESSION, "Compression error: the entropy kernels could not make progress") : rc;
}

} // namespace pixo_capi
