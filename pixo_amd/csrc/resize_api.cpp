// resize_api.cpp — the extern "C" resize entry points (pixo::resize, reference src/resize.rs): argument checks in the
// reference's order, the Lanczos3 contribution tables (built on the host once per call from resize_math.h, uploaded through
// the context's pinned staging), the launches of resize.hip.  The batch entries: the plan (tables shared between images of
// one size, sub-batches that bound the intermediate), one upload of tables and items, one launch per pass and sub-batch.
// The images entries: sources AND destinations of individual sizes and colour types, described by pixo_png_image records —
// the fitted sizes, the plan, the records of the flat launches (resize_images_math.h), one launch per pass and pixel size.
// The steps every batch driver takes, and their order: DESIGN.md §4.0; the shared ones: batch_steps.hpp.
#include "batch_steps.hpp"
#include "resize.hpp"
#include "resize_math.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <utility>
#include <vector>

using namespace pixo_capi;

namespace {

// resize_impl's checks (src/resize.rs:213-262), before any work.  data_len is checked unless `device` (a device pointer
// carries no length).
int resize_plan(const pixo_resize_options *o, bool device, size_t data_len, size_t *in_bytes, size_t *out_bytes)
{
    PIXO_REQUIRE(o);
    if (o->src_width == 0 || o->src_height == 0) return bad_dimensions(o->src_width, o->src_height);
    if (o->dst_width == 0 || o->dst_height == 0) return bad_dimensions(o->dst_width, o->dst_height);
    const uint32_t M = RZ_MAX_DIMENSION;
    if (o->src_width > M || o->src_height > M || o->dst_width > M || o->dst_height > M)
        return too_large(std::max(o->src_width, o->dst_width), std::max(o->src_height, o->dst_height), M);
    // (the C struct can carry codes the reference's enums cannot: answered like the flat entry's own checks)
    if (o->color_type > PIXO_RGBA) return bad_color_type(o->color_type);
    if (o->algorithm > PIXO_RESIZE_LANCZOS3)
        return fail(PIXO_ERR_INVALID_COLOR_ARG, "Invalid resize algorithm: " + std::to_string(o->algorithm) +
                                                    ". Expected 0 (Nearest), 1 (Bilinear), or 2 (Lanczos3)");
    const size_t bpp = bytes_per_pixel(o->color_type);
    *in_bytes = static_cast<size_t>(o->src_width) * o->src_height * bpp; // (2^24 * 2^24 * 4 fits 64 bits)
    *out_bytes = static_cast<size_t>(o->dst_width) * o->dst_height * bpp;
    return !device && data_len != *in_bytes ? bad_length(*in_bytes, data_len) : PIXO_OK;
}

// ---- contribution tables ----------------------------------------------------------------------------------------------------
// The number of weights of an axis and what fill_axis will return for it, without computing a weight (the batch plan: whether
// a tile fits the LDS segment)
void axis_measure(uint32_t src, uint32_t dst, size_t *total, uint32_t *max_span)
{
    const rz_axis a = rz_axis_of(src, dst);
    uint32_t span = 0, tile_lo = 0;
    size_t at = 0;
    for (uint32_t d = 0; d < dst; ++d) {
        uint32_t s, e;
        rz_taps(a, src, d, &s, &e);
        if (e < s) e = s;
        at += e - s;
        if (d % pixo_dev::kResizeHTile == 0) tile_lo = s;
        span = std::max(span, e - tile_lo);
    }
    *total = at;
    *max_span = span;
}
size_t axis_weights(uint32_t src, uint32_t dst)
{
    size_t total = 0;
    uint32_t span = 0;
    axis_measure(src, dst, &total, &span);
    return total;
}
// One axis as the kernels read it: start[dst], off[dst + 1] (u32), w[total] (f32); `total` from axis_weights
size_t axis_table_bytes(uint32_t dst, size_t total) { return ((static_cast<size_t>(dst) * 2 + 1 + total) * 4 + 15) & ~size_t{15}; }
// Fills the table at `base`; returns the widest source span of kResizeHTile adjacent destination indices.
uint32_t fill_axis(uint32_t src, uint32_t dst, uint8_t *base)
{
    const rz_axis a = rz_axis_of(src, dst);
    uint32_t *start = reinterpret_cast<uint32_t *>(base), *off = start + dst;
    float *w = reinterpret_cast<float *>(off + dst + 1);
    uint32_t at = 0, span = 0, tile_lo = 0;
    for (uint32_t d = 0; d < dst; ++d) {
        uint32_t s, e;
        rz_taps(a, src, d, &s, &e);
        if (e < s) e = s;
        start[d] = s;
        off[d] = at;
        rz_weights(a, d, s, e, w + at);
        at += e - s;
        if (d % pixo_dev::kResizeHTile == 0) tile_lo = s;
        span = std::max(span, e - tile_lo);
    }
    off[dst] = at;
    return span;
}
pixo_dev::ResizeAxisTable axis_on_device(const uint8_t *d_base, uint32_t dst)
{
    pixo_dev::ResizeAxisTable t;
    t.start = reinterpret_cast<const uint32_t *>(d_base);
    t.off = t.start + dst;
    t.w = reinterpret_cast<const float *>(t.off + dst + 1);
    return t;
}

// The tables of (src_w -> dst_w, src_h -> dst_h) in c.r_tables, uploaded on `s`; kept while the shape repeats.
int lanczos_tables(Context &c, const pixo_resize_options &o, hipStream_t s)
{
    const uint32_t want[4] = {o.src_width, o.dst_width, o.src_height, o.dst_height};
    if (c.r_tables.known == 1 && std::equal(want, want + 4, c.r_dims)) return PIXO_OK; // (a job of this context uploaded them: r_done exists)
    int rc = await_last_job(c.r_done); // (it reads r_tables, which go up from r_stage)
    if (rc) return rc;
    const size_t h_total = axis_weights(o.src_width, o.dst_width), v_total = axis_weights(o.src_height, o.dst_height);
    const size_t h_bytes = axis_table_bytes(o.dst_width, h_total), v_bytes = axis_table_bytes(o.dst_height, v_total);
    if (h_total > 0xFFFFFFFFull || v_total > 0xFFFFFFFFull) return fail(PIXO_ERR_COMPRESSION, "Compression error: contribution table too large");
    if ((rc = c.r_stage.reserve(h_bytes + v_bytes)) || (rc = c.r_tables.reserve(h_bytes + v_bytes))) return rc;
    c.r_tables.known = 0;
    uint8_t *stage = c.r_stage.as<uint8_t>();
    c.r_max_span = fill_axis(o.src_width, o.dst_width, stage);
    (void)fill_axis(o.src_height, o.dst_height, stage + h_bytes);
    HIP_TRY(hipMemcpyAsync(c.r_tables.p, stage, h_bytes + v_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c.r_done, s)); // (until the job's own record: the upload)
    std::copy(want, want + 4, c.r_dims);
    c.r_v_at = h_bytes;
    c.r_tables.known = 1;
    return PIXO_OK;
}

// Enqueues one resize on `s`: d_src -> d_dst (device pointers).
int resize_on_device(Context &c, const uint8_t *d_src, const pixo_resize_options &o, uint8_t *d_dst, hipStream_t s)
{
    const uint32_t bpp = bytes_per_pixel(o.color_type);
    if (o.algorithm != PIXO_RESIZE_LANCZOS3) {
        note_route(o.algorithm == PIXO_RESIZE_NEAREST ? route::RESIZE_NEAREST : route::RESIZE_BILINEAR);
        HIP_TRY(pixo_dev::launch_resize_point(d_src, o.src_width, o.src_height, d_dst, o.dst_width, o.dst_height, bpp, o.algorithm, s));
        return PIXO_OK;
    }
    note_route(route::RESIZE_LANCZOS3);
    // everything is reserved before any address is handed out (a growing reserve frees first: a device-wide wait)
    int rc;
    if ((rc = c.r_mid.reserve(pixo_dev::resize_mid_stride(o.dst_width, bpp) * o.src_height))) return rc;
    if ((rc = lanczos_tables(c, o, s))) return rc;
    HIP_TRY(hipStreamWaitEvent(s, c.r_done, 0)); // the intermediate is one per context: jobs on different streams take turns
    const uint8_t *tables = c.r_tables.as<uint8_t>();
    HIP_TRY(pixo_dev::launch_resize_lanczos_h(d_src, o.src_width, o.src_height, c.r_mid.as<uint8_t>(), o.dst_width, bpp,
                                              axis_on_device(tables, o.dst_width), c.r_max_span, s));
    HIP_TRY(pixo_dev::launch_resize_lanczos_v(c.r_mid.as<uint8_t>(), o.src_height, d_dst, o.dst_width, o.dst_height, bpp,
                                              axis_on_device(tables + c.r_v_at, o.dst_height), s));
    HIP_TRY(hipEventRecord(c.r_done, s));
    return PIXO_OK;
}

// Host pixels -> host storage of the caller's (out_bytes checked by the caller)
int resize_host(const uint8_t *data, size_t in_bytes, const pixo_resize_options &o, uint8_t *out, size_t out_bytes)
{
    PIXO_THREAD_CONTEXT(c);
    int rc;
    if ((rc = upload(c, c.r_in, data, in_bytes)) || (rc = reserve16(c.r_out, out_bytes))) return rc;
    if ((rc = resize_on_device(c, c.r_in.as<uint8_t>(), o, c.r_out.as<uint8_t>(), c.stream))) return rc;
    HIP_TRY(hipMemcpyAsync(out, c.r_out.p, out_bytes, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return PIXO_OK;
}

// ---- batches: n sources of individual sizes -> n images of one destination size --------------------------------------------
constexpr uint64_t kResizeBatchMidBytes = uint64_t{256} << 20; // Lanczos3 intermediate one sub-batch holds at most (debug switch resize_batch_bytes)
constexpr size_t kResizeBatchTableThreads = 8;                 // host threads that build a call's axis tables, at most ...
constexpr size_t kResizeBatchTableShare = size_t{128} << 10;   // ... one per this many bytes of tables (small batches: the calling thread alone)

// What the driver decided for a batch, before anything touches a device (also: pixo_hip_debug_resize_batch_plan).
struct BatchAxis {
    uint32_t src, dst;
    uint32_t max_span; // of a horizontal axis: the widest source span of one tile
    size_t at, bytes;  // its table in the block of tables
};
// The axis tables of a call: one per distinct (source, destination) pair per axis (a batch to one size: per distinct source
// width and per distinct source height)
struct AxisTables {
    std::vector<BatchAxis> axes;
    size_t table_bytes = 0; // all tables, each 16-byte aligned
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> h_of, v_of;
    // *index: the table of src -> dst among `axes`, measured and given its place when `seen` (h_of or v_of) has not met the pair
    int find(std::map<std::pair<uint32_t, uint32_t>, uint32_t> &seen, uint32_t src, uint32_t dst, uint32_t *index)
    {
        const auto found = seen.find({src, dst});
        if (found != seen.end()) { *index = found->second; return PIXO_OK; }
        size_t total = 0;
        uint32_t span = 0;
        axis_measure(src, dst, &total, &span);
        if (total > 0xFFFFFFFFull) return fail(PIXO_ERR_COMPRESSION, "Compression error: contribution table too large");
        const BatchAxis a{src, dst, span, table_bytes, axis_table_bytes(dst, total)};
        table_bytes += a.bytes;
        *index = seen[{src, dst}] = static_cast<uint32_t>(axes.size());
        axes.push_back(a);
        return PIXO_OK;
    }
};
// The tables at stage + axes[k].at.  The weights are host work (a sine in f64 each) and the axes are independent: a ragged batch,
// with up to two tables per image, builds them on several threads (64 x 1080p -> 320x180 of individual sizes: 7.4 ms on one)
void build_axis_tables(uint8_t *stage, const AxisTables &t)
{
    const unsigned builders = static_cast<unsigned>(std::min<size_t>({kResizeBatchTableThreads, t.axes.size(), t.table_bytes / kResizeBatchTableShare + 1}));
    run_on_threads(builders, [&](unsigned k) {
        for (size_t a = k; a < t.axes.size(); a += std::max(builders, 1u)) (void)fill_axis(t.axes[a].src, t.axes[a].dst, stage + t.axes[a].at);
    });
}
void note_resize_route(uint8_t algorithm, uint64_t entry, uint32_t subs)
{
    note_route((algorithm == PIXO_RESIZE_LANCZOS3 ? route::RESIZE_LANCZOS3 : algorithm == PIXO_RESIZE_NEAREST ? route::RESIZE_NEAREST : route::RESIZE_BILINEAR) |
               entry | (subs > 1 ? route::SUB_BATCHES : 0));
}
struct BatchPlan : AxisTables {
    SubBatches sub_first;
    std::vector<uint64_t> mid_at;         // per image: its rows' offset in the intermediate of its sub-batch
    std::vector<uint8_t> use_lds;         // per image: the horizontal pass stages in LDS
    std::vector<uint32_t> h_axis, v_axis; // per image: its axes in `axes`
    uint64_t mid_bytes = 0;               // the largest sub-batch's intermediate
};

// The sources have passed resize_plan's checks.  No HIP in here.
int resize_batch_plan(const pixo_resize_source *src, uint32_t batch, uint32_t dw, uint32_t dh, uint32_t bpp, uint8_t algorithm, BatchPlan &p)
{
    p.mid_at.assign(batch, 0);
    p.use_lds.assign(batch, 0);
    if (algorithm != PIXO_RESIZE_LANCZOS3) { // no tables, no intermediate: never cut
        p.sub_first.close(batch);
        return PIXO_OK;
    }
    p.h_axis.assign(batch, 0);
    p.v_axis.assign(batch, 0);
    const uint64_t limit = debug().resize_batch_bytes ? debug().resize_batch_bytes : kResizeBatchMidBytes;
    const uint64_t stride = pixo_dev::resize_mid_stride(dw, bpp);
    uint64_t held = 0; // the current sub-batch's intermediate so far
    for (uint32_t i = 0; i < batch; ++i) {
        int rc;
        if ((rc = p.find(p.h_of, src[i].width, dw, &p.h_axis[i])) || (rc = p.find(p.v_of, src[i].height, dh, &p.v_axis[i]))) return rc;
        p.use_lds[i] = pixo_dev::resize_h_uses_lds(p.axes[p.h_axis[i]].max_span, bpp);
        const uint64_t rows = stride * src[i].height; // (at most 2^26 * 2^24)
        if (p.sub_first.starts_at(i, held + rows > limit)) held = 0;
        p.mid_at[i] = held;
        held += rows;
        p.mid_bytes = std::max(p.mid_bytes, held);
    }
    p.sub_first.close(batch);
    return PIXO_OK;
}

// The checks of the batch entries up to the sources' own (the entries' pointers come behind them): sources, batch, then
// resize_plan's on (source i, destination) for i = 0, 1, ... with the single entry's status and its message + " (image i)".
int resize_batch_checks(const pixo_resize_source *sources, uint32_t batch, uint32_t dw, uint32_t dh, uint8_t color_type, uint8_t algorithm,
                        size_t *out_bytes)
{
    PIXO_REQUIRE(sources);
    int rc = batch_in_range(batch);
    if (rc) return rc;
    for (uint32_t i = 0; i < batch; ++i) {
        pixo_resize_options o;
        o.src_width = sources[i].width; o.src_height = sources[i].height;
        o.dst_width = dw; o.dst_height = dh;
        o.color_type = color_type; o.algorithm = algorithm;
        size_t in_bytes = 0;
        if ((rc = resize_plan(&o, true, 0, &in_bytes, out_bytes))) return fail(rc, t_error + where(i));
    }
    if (*out_bytes > (size_t{1} << 62) / batch) return fail(PIXO_ERR_COMPRESSION, "Compression error: batch output too large");
    return PIXO_OK;
}
int resize_batch_pixels_given(const pixo_resize_source *sources, uint32_t batch)
{
    for (uint32_t i = 0; i < batch; ++i)
        if (!sources[i].pixels) return fail(PIXO_ERR_COMPRESSION, "Compression error: null argument 'pixels'" + where(i));
    return PIXO_OK;
}

// Enqueues one batch on `s`: sources[i].pixels (device pointers) -> d_dst + i * out_bytes.  The tables and the items go up in one
// copy; the sub-batches follow each other on `s`, so the intermediate is reused in stream order.
int resize_batch_on_device(Context &c, const pixo_resize_source *sources, uint32_t batch, uint32_t dw, uint32_t dh, uint8_t color_type,
                           uint8_t algorithm, uint8_t *d_dst, hipStream_t s)
{
    const uint32_t bpp = bytes_per_pixel(color_type);
    const size_t out_bytes = static_cast<size_t>(dw) * dh * bpp;
    BatchPlan p;
    int rc = resize_batch_plan(sources, batch, dw, dh, bpp, algorithm, p);
    if (rc) return rc;
    const bool lanczos = algorithm == PIXO_RESIZE_LANCZOS3;
    const uint32_t subs = p.sub_first.count();
    note_resize_route(algorithm, route::RESIZE_BATCH, subs);
    if ((rc = await_last_job(c.rb_done))) return rc; // (it reads rb_tables, which go up from rb_stage)
    // everything is reserved before any address is handed out (a growing reserve frees first: a device-wide wait)
    const size_t up_bytes = p.table_bytes + static_cast<size_t>(batch) * sizeof(pixo_dev::ResizeBatchItem);
    if ((rc = c.rb_stage.reserve(up_bytes)) || (rc = c.rb_tables.reserve(up_bytes)) || (rc = c.rb_mid.reserve(p.mid_bytes))) return rc;
    uint8_t *stage = c.rb_stage.as<uint8_t>();
    build_axis_tables(stage, p);
    pixo_dev::ResizeBatchItem *items = reinterpret_cast<pixo_dev::ResizeBatchItem *>(stage + p.table_bytes); // (table_bytes is a multiple of 16)
    for (uint32_t i = 0; i < batch; ++i) {
        pixo_dev::ResizeBatchItem &it = items[i];
        it.src = static_cast<const uint8_t *>(sources[i].pixels);
        it.mid_at = p.mid_at[i];
        it.h_at = lanczos ? p.axes[p.h_axis[i]].at : 0;
        it.v_at = lanczos ? p.axes[p.v_axis[i]].at : 0;
        it.sw = sources[i].width; it.sh = sources[i].height;
        it.use_lds = p.use_lds[i];
        it.reserved = 0;
    }
    HIP_TRY(hipMemcpyAsync(c.rb_tables.p, stage, up_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c.rb_done, s)); // (until the job's own record: the upload)
    const uint8_t *d_tables = c.rb_tables.as<uint8_t>();
    const pixo_dev::ResizeBatchItem *d_items = reinterpret_cast<const pixo_dev::ResizeBatchItem *>(d_tables + p.table_bytes);
    for (uint32_t k = 0; k < subs; ++k) {
        const uint32_t first = p.sub_first[k], n = p.sub_first[k + 1] - first;
        uint8_t *out = d_dst + static_cast<size_t>(first) * out_bytes;
        if (!lanczos) {
            HIP_TRY(pixo_dev::launch_resize_point_batch(d_items + first, n, out, dw, dh, bpp, algorithm, s));
            continue;
        }
        uint32_t max_sh = 0;
        for (uint32_t i = first; i < first + n; ++i) max_sh = std::max(max_sh, sources[i].height);
        HIP_TRY(pixo_dev::launch_resize_lanczos_h_batch(d_items + first, n, max_sh, d_tables, c.rb_mid.as<uint8_t>(), dw, bpp, s));
        HIP_TRY(pixo_dev::launch_resize_lanczos_v_batch(d_items + first, n, d_tables, c.rb_mid.as<uint8_t>(), out, dw, dh, bpp, s));
    }
    HIP_TRY(hipEventRecord(c.rb_done, s));
    return PIXO_OK;
}

// ---- images: n sources of individual sizes and colour types -> n images of individual sizes, anywhere in one block ----------
namespace rzi = pixo_resize_images;

// JavaScript's Math.round for x >= 0: the nearest integer, a tie towards +infinity (x - floor(x) is exact in f64)
double js_round(double x)
{
    const double f = std::floor(x);
    return x - f >= 0.5 ? f + 1.0 : f;
}
// The largest size of (sw, sh)'s proportions inside the box, as the reference's front end computes it (web/src/lib/wasm.ts
// calculateResizeDimensions): the box's width and the height that goes with it; if that is too tall, the box's height and
// the width that goes with it.  f64 throughout, each side at least 1; neither side exceeds the box's.
void fit_size(uint32_t sw, uint32_t sh, uint32_t box_w, uint32_t box_h, uint32_t *dw, uint32_t *dh)
{
    const double aspect = static_cast<double>(sw) / static_cast<double>(sh);
    double w = box_w, h = js_round(static_cast<double>(box_w) / aspect);
    if (h > static_cast<double>(box_h)) {
        h = box_h;
        w = js_round(static_cast<double>(box_h) * aspect);
    }
    *dw = static_cast<uint32_t>(std::max(1.0, w));
    *dh = static_cast<uint32_t>(std::max(1.0, h));
}

// What the driver decided for the images, before anything touches a device (also: pixo_hip_debug_resize_images_plan).
struct ImagesPlan : AxisTables {
    SubBatches sub_first;
    std::vector<uint64_t> mid_at;                    // per image: its rows' offset in the intermediate of its sub-batch
    std::vector<uint8_t> use_lds;                    // per image: the horizontal pass stages in LDS
    std::vector<uint32_t> h_axis, v_axis;            // per image: its axes in `axes`
    std::vector<uint32_t> tiles_first, tiles_second; // per image: its tiles in the point / horizontal pass, in the vertical pass
    uint64_t mid_bytes = 0;                          // the largest sub-batch's intermediate
    uint32_t launches_first = 0, launches_second = 0; // launches of the two passes, summed over the sub-batches
    uint32_t rows_cap = rzi::kRowsCap;
};

// The images have passed resize_images_checks.  No HIP in here.
int resize_images_plan(const pixo_png_image *src, const pixo_png_image *dst, uint32_t batch, uint8_t algorithm, ImagesPlan &p)
{
    const bool lanczos = algorithm == PIXO_RESIZE_LANCZOS3;
    p.rows_cap = debug().resize_images_rows ? debug().resize_images_rows : rzi::kRowsCap;
    p.mid_at.assign(batch, 0);
    p.use_lds.assign(batch, 0);
    p.h_axis.assign(batch, 0);
    p.v_axis.assign(batch, 0);
    p.tiles_first.assign(batch, 0);
    p.tiles_second.assign(batch, 0);
    const uint64_t limit = debug().resize_batch_bytes ? debug().resize_batch_bytes : kResizeBatchMidBytes;
    uint64_t held = 0;                     // the current sub-batch's intermediate so far
    uint64_t first[5] = {0, 0, 0, 0, 0};   // ... the tiles of its point / horizontal launches so far, by bytes per pixel
    uint64_t second = 0;                   // ... of its vertical launch
    for (uint32_t i = 0; i < batch; ++i) {
        const uint32_t bpp = bytes_per_pixel(src[i].color_type);
        uint64_t rows = 0;
        if (lanczos) {
            int rc;
            if ((rc = p.find(p.h_of, src[i].width, dst[i].width, &p.h_axis[i])) || (rc = p.find(p.v_of, src[i].height, dst[i].height, &p.v_axis[i]))) return rc;
            p.use_lds[i] = pixo_dev::resize_h_uses_lds(p.axes[p.h_axis[i]].max_span, bpp);
            rows = static_cast<uint64_t>(pixo_dev::resize_mid_stride(dst[i].width, bpp)) * src[i].height; // (at most 2^26 * 2^24)
        }
        const uint64_t a = rzi::tile_count(lanczos ? rzi::PASS_H : rzi::PASS_POINT, src[i].height, dst[i].width, dst[i].height, bpp, p.rows_cap);
        const uint64_t b = lanczos ? rzi::tile_count(rzi::PASS_V, src[i].height, dst[i].width, dst[i].height, bpp, p.rows_cap) : 0;
        // a launch's tiles stay within 31 bits (one image's do: tiles_of)
        if (p.sub_first.starts_at(i, held + rows > limit || first[bpp] + a > rzi::kMaxTiles || second + b > rzi::kMaxTiles)) {
            held = second = 0;
            std::fill(first, first + 5, uint64_t{0});
        }
        if (first[bpp] == 0) p.launches_first += 1;
        if (lanczos && second == 0) p.launches_second += 1;
        p.mid_at[i] = held;
        p.tiles_first[i] = static_cast<uint32_t>(a);
        p.tiles_second[i] = static_cast<uint32_t>(b);
        held += rows;
        first[bpp] += a;
        second += b;
        p.mid_bytes = std::max(p.mid_bytes, held);
    }
    p.sub_first.close(batch);
    return PIXO_OK;
}

// The checks the images entries share, in their order (include/pixo_hip.h).  *src_end / *dst_end: the furthest image's end.
int resize_images_checks(const pixo_png_image *src_images, const pixo_png_image *dst_images, uint32_t batch, uint8_t algorithm, uint64_t *src_end,
                         uint64_t *dst_end)
{
    PIXO_REQUIRE(src_images);
    PIXO_REQUIRE(dst_images);
    int rc = batch_in_range(batch);
    if (rc) return rc;
    *src_end = *dst_end = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        const std::string here = where(i);
        const pixo_png_image &a = src_images[i], &b = dst_images[i];
        pixo_resize_options o;
        o.src_width = a.width; o.src_height = a.height;
        o.dst_width = b.width; o.dst_height = b.height;
        o.color_type = a.color_type; o.algorithm = algorithm;
        size_t in_bytes = 0, out_bytes = 0;
        if ((rc = resize_plan(&o, true, 0, &in_bytes, &out_bytes))) return fail(rc, t_error + here);
        if (b.color_type != a.color_type) return fail(PIXO_ERR_COMPRESSION, "Compression error: colour types differ" + here);
        if ((rc = record_extent(a.offset, in_bytes, "input", here, src_end)) || (rc = record_extent(b.offset, out_bytes, "output", here, dst_end))) return rc;
    }
    return PIXO_OK;
}

// Enqueues the images on `s`: d_src + src[i].offset -> d_dst + dst[i].offset.  The tables and the records of every pass and
// sub-batch go up in one copy; the sub-batches follow each other on `s`, so the intermediate is reused in stream order.
// Shares the batch entries' buffers and their event: the two kinds of job take turns as two batches do.
int resize_images_on_device(Context &c, const uint8_t *d_src, const pixo_png_image *src, uint8_t *d_dst, const pixo_png_image *dst, uint32_t batch,
                            uint8_t algorithm, hipStream_t s)
{
    ImagesPlan p;
    int rc = resize_images_plan(src, dst, batch, algorithm, p);
    if (rc) return rc;
    const bool lanczos = algorithm == PIXO_RESIZE_LANCZOS3;
    const uint32_t subs = p.sub_first.count(), passes = lanczos ? 2 : 1;
    note_resize_route(algorithm, route::RESIZE_IMAGES, subs);
    if ((rc = await_last_job(c.rb_done))) return rc; // (it reads rb_tables, which go up from rb_stage)
    // everything is reserved before any address is handed out (a growing reserve frees first: a device-wide wait)
    const size_t up_bytes = p.table_bytes + static_cast<size_t>(passes) * batch * sizeof(rzi::Record);
    if ((rc = c.rb_stage.reserve(up_bytes)) || (rc = c.rb_tables.reserve(up_bytes)) || (rc = c.rb_mid.reserve(p.mid_bytes))) return rc;
    uint8_t *stage = c.rb_stage.as<uint8_t>();
    build_axis_tables(stage, p);
    // the records: pass after pass, inside a pass sub-batch after sub-batch (table_bytes is a multiple of 16)
    rzi::Record *records = reinterpret_cast<rzi::Record *>(stage + p.table_bytes);
    struct Enqueued {
        rzi::Launch l;
        int pass;
        size_t first_record; // in `records`
    };
    std::vector<Enqueued> launches;
    std::vector<rzi::Item> items;
    std::vector<rzi::Record> table;
    std::vector<rzi::Launch> of_pass;
    std::vector<uint32_t> record_item;
    for (uint32_t k = 0; k < subs; ++k) {
        const uint32_t first = p.sub_first[k], n = p.sub_first[k + 1] - first;
        items.clear();
        for (uint32_t i = first; i < first + n; ++i) {
            const uint32_t bpp = bytes_per_pixel(src[i].color_type);
            items.push_back(rzi::Item{reinterpret_cast<uint64_t>(d_src) + src[i].offset, reinterpret_cast<uint64_t>(d_dst) + dst[i].offset, p.mid_at[i],
                                      lanczos ? pixo_dev::resize_mid_stride(dst[i].width, bpp) : 0, lanczos ? p.axes[p.h_axis[i]].at : 0,
                                      lanczos ? p.axes[p.v_axis[i]].at : 0, src[i].width, src[i].height, dst[i].width, dst[i].height, bpp, p.use_lds[i]});
        }
        for (uint32_t pass = 0; pass < passes; ++pass) {
            const int which = !lanczos ? rzi::PASS_POINT : pass == 0 ? rzi::PASS_H : rzi::PASS_V;
            if (!rzi::build_table(items, which, p.rows_cap, table, of_pass, record_item))
                return fail(PIXO_ERR_COMPRESSION, "Compression error: resize launch too large"); // (the plan cuts before that)
            const size_t at = static_cast<size_t>(pass) * batch + first;
            std::copy(table.begin(), table.end(), records + at);
            for (const rzi::Launch &l : of_pass) launches.push_back(Enqueued{l, which, at + l.first_record});
        }
    }
    HIP_TRY(hipMemcpyAsync(c.rb_tables.p, stage, up_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c.rb_done, s)); // (until the job's own record: the upload)
    const uint8_t *d_tables = c.rb_tables.as<uint8_t>();
    const rzi::Record *d_records = reinterpret_cast<const rzi::Record *>(d_tables + p.table_bytes);
    for (const Enqueued &e : launches) { // (in the order built: a sub-batch's horizontal launches, its vertical one, the next sub-batch's)
        const rzi::Record *r = d_records + e.first_record;
        if (e.pass == rzi::PASS_POINT) HIP_TRY(pixo_dev::launch_resize_point_images(r, e.l.count, e.l.tiles, e.l.bpp, algorithm, s));
        else if (e.pass == rzi::PASS_H)
            HIP_TRY(pixo_dev::launch_resize_lanczos_h_images(r, e.l.count, e.l.tiles, d_tables, c.rb_mid.as<uint8_t>(), e.l.bpp, s));
        else HIP_TRY(pixo_dev::launch_resize_lanczos_v_images(r, e.l.count, e.l.tiles, d_tables, c.rb_mid.as<uint8_t>(), s));
    }
    HIP_TRY(hipEventRecord(c.rb_done, s));
    return PIXO_OK;
}

} // namespace

extern "C" {

int pixo_hip_resize_images_fit(const pixo_png_image *src_images, uint32_t batch, uint32_t box_width, uint32_t box_height, uint32_t flags,
                               pixo_png_image *dst_images, size_t *total)
{
    PIXO_REQUIRE(src_images);
    PIXO_REQUIRE(dst_images);
    PIXO_REQUIRE(total);
    int rc = batch_in_range(batch);
    if (rc) return rc;
    if (box_width == 0 || box_height == 0) return bad_dimensions(box_width, box_height);
    if (box_width > RZ_MAX_DIMENSION || box_height > RZ_MAX_DIMENSION) return too_large(box_width, box_height, RZ_MAX_DIMENSION);
    for (uint32_t i = 0; i < batch; ++i) { // nothing is written before every image has passed
        const pixo_png_image &a = src_images[i];
        if (a.width == 0 || a.height == 0) { rc = bad_dimensions(a.width, a.height); return fail(rc, t_error + where(i)); }
        if (a.width > RZ_MAX_DIMENSION || a.height > RZ_MAX_DIMENSION) { rc = too_large(a.width, a.height, RZ_MAX_DIMENSION); return fail(rc, t_error + where(i)); }
        if (a.color_type > PIXO_RGBA) return bad_color_type(a.color_type, where(i));
    }
    uint64_t at = 0, end = 0;
    std::vector<pixo_png_image> fitted(batch); // (dst_images may be src_images)
    for (uint32_t i = 0; i < batch; ++i) {
        const pixo_png_image &a = src_images[i];
        uint32_t w = a.width, h = a.height;
        if (!(flags & PIXO_RESIZE_FIT_NO_ENLARGE) || w > box_width || h > box_height) fit_size(a.width, a.height, box_width, box_height, &w, &h);
        fitted[i] = lay_out(at, w, h, a.color_type, &end); // (at most 2^16 images of 2^50 bytes: below 2^64)
    }
    if (end > (uint64_t{1} << 62)) return fail(PIXO_ERR_COMPRESSION, "Compression error: batch output too large");
    report(fitted, dst_images);
    *total = static_cast<size_t>(end);
    return PIXO_OK;
}

int pixo_hip_resize_images_device(const void *d_src, const pixo_png_image *src_images, void *d_dst, const pixo_png_image *dst_images, uint32_t batch,
                                  uint8_t algorithm, void *stream)
{
    uint64_t src_end = 0, dst_end = 0;
    int rc = resize_images_checks(src_images, dst_images, batch, algorithm, &src_end, &dst_end);
    if (rc) return rc;
    PIXO_REQUIRE(d_src);
    PIXO_REQUIRE(d_dst);
    PIXO_CALLER_STREAM_CONTEXT(c, s, stream);
    return resize_images_on_device(*c, static_cast<const uint8_t *>(d_src), src_images, static_cast<uint8_t *>(d_dst), dst_images, batch, algorithm, s);
}

int pixo_hip_resize_images(const uint8_t *data, size_t data_len, const pixo_png_image *src_images, const pixo_png_image *dst_images, uint32_t batch,
                           uint8_t algorithm, uint8_t **out, size_t *out_len)
{
    uint64_t src_end = 0, dst_end = 0;
    int rc = resize_images_checks(src_images, dst_images, batch, algorithm, &src_end, &dst_end);
    if (rc) return rc;
    PIXO_REQUIRE(data);
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    if (data_len < src_end) return bad_length(static_cast<size_t>(src_end), data_len);
    PIXO_THREAD_CONTEXT(c);
    if ((rc = upload(c, c.rb_in, data, static_cast<size_t>(src_end))) || (rc = reserve16(c.rb_out, static_cast<size_t>(dst_end)))) return rc;
    uint8_t *block = alloc_file(static_cast<size_t>(dst_end));
    if (!block) return fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
    rc = resize_images_on_device(c, c.rb_in.as<uint8_t>(), src_images, c.rb_out.as<uint8_t>(), dst_images, batch, algorithm, c.stream);
    return download_block(c, rc, block, c.rb_out.p, static_cast<size_t>(dst_end), out, out_len);
}

int pixo_hip_debug_resize_images_plan(const pixo_png_image *src_images, const pixo_png_image *dst_images, uint32_t batch, uint8_t algorithm,
                                      uint32_t *sub_first, uint32_t *sub_count, uint64_t *mid_at, uint8_t *use_lds, uint32_t *tiles_first,
                                      uint32_t *tiles_second, uint32_t *axis_tables, uint32_t *launches_first, uint32_t *launches_second)
{
    uint64_t src_end = 0, dst_end = 0;
    int rc = resize_images_checks(src_images, dst_images, batch, algorithm, &src_end, &dst_end);
    if (rc) return rc;
    PIXO_REQUIRE(sub_first);
    PIXO_REQUIRE(sub_count);
    PIXO_REQUIRE(mid_at);
    PIXO_REQUIRE(use_lds);
    PIXO_REQUIRE(tiles_first);
    PIXO_REQUIRE(tiles_second);
    PIXO_REQUIRE(axis_tables);
    PIXO_REQUIRE(launches_first);
    PIXO_REQUIRE(launches_second);
    ImagesPlan p;
    if ((rc = resize_images_plan(src_images, dst_images, batch, algorithm, p))) return rc;
    p.sub_first.report(sub_first, sub_count);
    std::copy(p.mid_at.begin(), p.mid_at.end(), mid_at);
    std::copy(p.use_lds.begin(), p.use_lds.end(), use_lds);
    std::copy(p.tiles_first.begin(), p.tiles_first.end(), tiles_first);
    std::copy(p.tiles_second.begin(), p.tiles_second.end(), tiles_second);
    *axis_tables = static_cast<uint32_t>(p.axes.size());
    *launches_first = p.launches_first;
    *launches_second = p.launches_second;
    return PIXO_OK;
}

int pixo_hip_resize_batch_device(const pixo_resize_source *sources, uint32_t batch, uint32_t dst_width, uint32_t dst_height, uint8_t color_type,
                                 uint8_t algorithm, void *d_dst, void *stream)
{
    size_t out_bytes = 0;
    int rc = resize_batch_checks(sources, batch, dst_width, dst_height, color_type, algorithm, &out_bytes);
    if (rc || (rc = resize_batch_pixels_given(sources, batch))) return rc;
    PIXO_REQUIRE(d_dst);
    PIXO_CALLER_STREAM_CONTEXT(c, s, stream);
    return resize_batch_on_device(*c, sources, batch, dst_width, dst_height, color_type, algorithm, static_cast<uint8_t *>(d_dst), s);
}

int pixo_hip_resize_batch(const pixo_resize_source *sources, uint32_t batch, uint32_t dst_width, uint32_t dst_height, uint8_t color_type,
                          uint8_t algorithm, uint8_t **out, size_t *out_len)
{
    size_t out_bytes = 0;
    int rc = resize_batch_checks(sources, batch, dst_width, dst_height, color_type, algorithm, &out_bytes);
    if (rc || (rc = resize_batch_pixels_given(sources, batch))) return rc;
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    const size_t bpp = bytes_per_pixel(color_type), all_out = out_bytes * batch;
    std::vector<pixo_resize_source> on_device(sources, sources + batch);
    std::vector<size_t> at(batch + 1, 0); // every source starts at a multiple of 16 in rb_in
    for (uint32_t i = 0; i < batch; ++i) at[i + 1] = at[i] + ((static_cast<size_t>(sources[i].width) * sources[i].height * bpp + 15) & ~size_t{15});
    PIXO_THREAD_CONTEXT(c);
    if ((rc = c.rb_in.reserve(at[batch])) || (rc = reserve16(c.rb_out, all_out))) return rc;
    for (uint32_t i = 0; i < batch; ++i) {
        on_device[i].pixels = c.rb_in.as<uint8_t>() + at[i];
        HIP_TRY(hipMemcpyAsync(c.rb_in.as<uint8_t>() + at[i], sources[i].pixels, static_cast<size_t>(sources[i].width) * sources[i].height * bpp,
                               hipMemcpyHostToDevice, c.stream));
    }
    uint8_t *block = alloc_file(all_out);
    if (!block) return fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
    rc = resize_batch_on_device(c, on_device.data(), batch, dst_width, dst_height, color_type, algorithm, c.rb_out.as<uint8_t>(), c.stream);
    return download_block(c, rc, block, c.rb_out.p, all_out, out, out_len);
}

int pixo_hip_debug_resize_batch_plan(const pixo_resize_source *sources, uint32_t batch, uint32_t dst_width, uint32_t dst_height, uint8_t color_type,
                                     uint8_t algorithm, uint32_t *sub_first, uint32_t *sub_count, uint64_t *mid_at, uint8_t *use_lds,
                                     uint32_t *axis_tables)
{
    size_t out_bytes = 0;
    int rc = resize_batch_checks(sources, batch, dst_width, dst_height, color_type, algorithm, &out_bytes);
    if (rc) return rc;
    PIXO_REQUIRE(sub_first);
    PIXO_REQUIRE(sub_count);
    PIXO_REQUIRE(mid_at);
    PIXO_REQUIRE(use_lds);
    PIXO_REQUIRE(axis_tables);
    BatchPlan p;
    if ((rc = resize_batch_plan(sources, batch, dst_width, dst_height, bytes_per_pixel(color_type), algorithm, p))) return rc;
    p.sub_first.report(sub_first, sub_count);
    std::copy(p.mid_at.begin(), p.mid_at.end(), mid_at);
    std::copy(p.use_lds.begin(), p.use_lds.end(), use_lds);
    *axis_tables = static_cast<uint32_t>(p.axes.size());
    return PIXO_OK;
}

int pixo_hip_resize_into(uint8_t *output, size_t capacity, const uint8_t *data, size_t data_len, const pixo_resize_options *options,
                         size_t *out_len)
{
    CallerStorageScope storage(true);
    PIXO_REQUIRE(out_len);
    size_t in_bytes = 0, out_bytes = 0;
    int rc = resize_plan(options, false, data_len, &in_bytes, &out_bytes);
    if (rc) return rc;
    *out_len = out_bytes;
    if (capacity < out_bytes) return too_small(out_bytes);
    PIXO_REQUIRE(data);
    PIXO_REQUIRE(output);
    return resize_host(data, in_bytes, *options, output, out_bytes);
}

int pixo_hip_resize(const uint8_t *data, size_t data_len, const pixo_resize_options *options, uint8_t **out, size_t *out_len)
{
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    size_t in_bytes = 0, out_bytes = 0;
    int rc = resize_plan(options, false, data_len, &in_bytes, &out_bytes);
    if (rc) return rc;
    PIXO_REQUIRE(data);
    uint8_t *block = alloc_file(out_bytes);
    if (!block) return fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
    if ((rc = resize_host(data, in_bytes, *options, block, out_bytes))) { free_file(block); return rc; }
    *out = block;
    *out_len = out_bytes;
    return PIXO_OK;
}

int pixo_hip_resize_image(const uint8_t *data, size_t data_len, uint32_t src_width, uint32_t src_height, uint32_t dst_width,
                          uint32_t dst_height, uint8_t color_type, uint8_t algorithm, uint8_t **out, size_t *out_len)
{ // wasm.rs:183-201: color_type_from_u8, then resize_algorithm_from_u8, then the builder
    if (color_type > PIXO_RGBA) return bad_color_type(color_type);
    if (algorithm > PIXO_RESIZE_LANCZOS3)
        return fail(PIXO_ERR_INVALID_COLOR_ARG, "Invalid resize algorithm: " + std::to_string(algorithm) +
                                                    ". Expected 0 (Nearest), 1 (Bilinear), or 2 (Lanczos3)");
    pixo_resize_options o;
    o.src_width = src_width; o.src_height = src_height;
    o.dst_width = dst_width; o.dst_height = dst_height;
    o.color_type = color_type; o.algorithm = algorithm;
    return pixo_hip_resize(data, data_len, &o, out, out_len);
}

int pixo_hip_resize_device(const void *d_src, const pixo_resize_options *options, void *d_dst, void *stream)
{
    size_t in_bytes = 0, out_bytes = 0;
    int rc = resize_plan(options, true, 0, &in_bytes, &out_bytes);
    if (rc) return rc;
    PIXO_REQUIRE(d_src);
    PIXO_REQUIRE(d_dst);
    PIXO_CALLER_STREAM_CONTEXT(c, s, stream);
    return resize_on_device(*c, static_cast<const uint8_t *>(d_src), *options, static_cast<uint8_t *>(d_dst), s);
}

int pixo_hip_resize_contributions(uint32_t src, uint32_t dst, uint32_t *starts, uint32_t *counts, float *weights, size_t capacity,
                                  size_t *total)
{
    PIXO_REQUIRE(total);
    if (src == 0 || dst == 0) return bad_dimensions(src, dst);
    if (src > RZ_MAX_DIMENSION || dst > RZ_MAX_DIMENSION) return too_large(src, dst, RZ_MAX_DIMENSION);
    *total = axis_weights(src, dst);
    if (capacity < *total) return fail(PIXO_ERR_BUFFER_TOO_SMALL, "output buffer too small: need " + std::to_string(*total) + " weights");
    PIXO_REQUIRE(starts);
    PIXO_REQUIRE(counts);
    PIXO_REQUIRE(weights);
    const rz_axis a = rz_axis_of(src, dst);
    size_t at = 0;
    for (uint32_t d = 0; d < dst; ++d) {
        uint32_t s, e;
        rz_taps(a, src, d, &s, &e);
        if (e < s) e = s;
        starts[d] = s;
        counts[d] = e - s;
        rz_weights(a, d, s, e, weights + at);
        at += e - s;
    }
    return PIXO_OK;
}

} // extern "C"
