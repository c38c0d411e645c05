// resize_api.cpp — the extern "C" resize entry points (pixo::resize, reference src/resize.rs): argument checks in the
// reference's order, the Lanczos3 contribution tables (built on the host once per call from resize_math.h, uploaded through
// the context's pinned staging), the launches of resize.hip.
#include "capi_internal.hpp"
#include "resize.hpp"
#include "resize_math.h"

#include <algorithm>
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
    if (o->color_type > PIXO_RGBA)
        return fail(PIXO_ERR_INVALID_COLOR_ARG, "Invalid color type: " + std::to_string(o->color_type) +
                                                    ". Expected 0 (Gray), 1 (GrayAlpha), 2 (Rgb), or 3 (Rgba)");
    if (o->algorithm > PIXO_RESIZE_LANCZOS3)
        return fail(PIXO_ERR_INVALID_COLOR_ARG, "Invalid resize algorithm: " + std::to_string(o->algorithm) +
                                                    ". Expected 0 (Nearest), 1 (Bilinear), or 2 (Lanczos3)");
    const size_t bpp = bytes_per_pixel(o->color_type);
    *in_bytes = static_cast<size_t>(o->src_width) * o->src_height * bpp; // (2^24 * 2^24 * 4 fits 64 bits)
    *out_bytes = static_cast<size_t>(o->dst_width) * o->dst_height * bpp;
    return !device && data_len != *in_bytes ? bad_length(*in_bytes, data_len) : PIXO_OK;
}

// ---- contribution tables ----------------------------------------------------------------------------------------------------
size_t axis_weights(uint32_t src, uint32_t dst)
{
    const rz_axis a = rz_axis_of(src, dst);
    size_t total = 0;
    for (uint32_t d = 0; d < dst; ++d) {
        uint32_t s, e;
        rz_taps(a, src, d, &s, &e);
        total += e > s ? e - s : 0;
    }
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
    if (!c.r_done) HIP_TRY(hipEventCreateWithFlags(&c.r_done, hipEventDisableTiming));
    const uint32_t want[4] = {o.src_width, o.dst_width, o.src_height, o.dst_height};
    if (c.r_tables.known == 1 && std::equal(want, want + 4, c.r_dims)) return PIXO_OK;
    // the job before may still be reading the tables, and the staging may still be on its way: both are about to change
    HIP_TRY(hipEventSynchronize(c.r_done));
    const size_t h_total = axis_weights(o.src_width, o.dst_width), v_total = axis_weights(o.src_height, o.dst_height);
    const size_t h_bytes = axis_table_bytes(o.dst_width, h_total), v_bytes = axis_table_bytes(o.dst_height, v_total);
    if (h_total > 0xFFFFFFFFull || v_total > 0xFFFFFFFFull) return fail(PIXO_ERR_COMPRESSION, "Compression error: contribution table too large");
    int rc;
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

} // namespace

extern "C" {

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
    if (color_type > PIXO_RGBA)
        return fail(PIXO_ERR_INVALID_COLOR_ARG, "Invalid color type: " + std::to_string(color_type) +
                                                    ". Expected 0 (Gray), 1 (GrayAlpha), 2 (Rgb), or 3 (Rgba)");
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
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc; // (records the producer stream's event)
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (c->producer_done) HIP_TRY(hipStreamWaitEvent(s, c->producer_done, 0));
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
