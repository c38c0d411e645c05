// jpeg_api.cpp — the extern "C" JPEG entry points declared in include/pixo_hip.h: check the arguments (each entry in its own
// order), find the context, encode_file, deliver (file_route.cpp).  No CPU fallback exists: without a usable GPU every compute
// entry point fails with PIXO_ERR_COMPRESSION and says so.
#include "dispatch_gate.hpp"
#include "capi_internal.hpp"

using namespace pixo_capi;

namespace {
int fail_tuple_trellis()
{ // trellis quantisation happens between the transform and the tuple (src/jpeg/mod.rs:932-976): a tuple entry cannot apply it
    return fail(PIXO_ERR_COMPRESSION, "Compression error: trellis_quant needs the pixels: quantise the tuple with the trellis "
                                      "quantiser first and clear the flag, or use an entry point that takes pixels");
}
pixo_jpeg_options flat_options(uint32_t width, uint32_t height, uint8_t color_type, uint8_t subsampling, uint8_t quality)
{
    pixo_jpeg_options o{};
    o.width = width; o.height = height; o.color_type = color_type; o.quality = quality; o.subsampling = subsampling;
    return o;
}
// The host arrays of a tuple entry: their sizes (the reference's length error), then the pointers
int tuple_arrays_checked(const pixo_host::Geometry &g, const uint8_t *pixels, const int16_t *y, size_t y_blocks, const int16_t *cb,
                         const int16_t *cr, size_t c_blocks)
{
    if (y_blocks != g.y_blocks || c_blocks != g.c_blocks)
        return fail(PIXO_ERR_INVALID_DATA_LENGTH, "Invalid pixel data length: expected " + std::to_string(g.y_blocks) + " bytes, got " +
                                                      std::to_string(y_blocks));
    PIXO_REQUIRE(pixels);
    PIXO_REQUIRE(y);
    if (g.c_blocks && (!cb || !cr)) return fail(PIXO_ERR_COMPRESSION, "Compression error: null argument 'cb'/'cr'");
    return PIXO_OK;
}
// What the tuple -> file entries check in front of their tuple pointer
int tuple_entry_checked(const pixo_jpeg_options *options, uint8_t **out, size_t *out_len)
{
    PIXO_REQUIRE(options);
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    if (const int rc = checked(*options)) return rc;
    return options->progressive && options->trellis_quant ? fail_tuple_trellis() : PIXO_OK;
}
} // namespace

extern "C" {

void pixo_jpeg_options_from_preset(pixo_jpeg_options *o, uint32_t width, uint32_t height,
                                   uint8_t quality, uint8_t preset)
{ // jpeg/mod.rs:162-216
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->width = width; o->height = height; o->color_type = PIXO_RGB; o->quality = quality;
    o->subsampling = PIXO_S444;
    if (preset == 0) return;
    o->optimize_huffman = 1;
    if (preset == 2) { o->subsampling = PIXO_S420; o->progressive = 1; o->trellis_quant = 1; }
}

int pixo_hip_jpeg_encode(const uint8_t *data, size_t data_len, const pixo_jpeg_options *options,
                         uint8_t **out, size_t *out_len)
{
    PIXO_REQUIRE(options);
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    if (const int rc = checked(*options, true, data_len)) return rc;
    PIXO_REQUIRE(data);
    FileResult r;
    const int rc = encode_host_pixels(data, *options, FileDest::own_block(), r);
    return rc ? rc : deliver_block(r, out, out_len);
}

int pixo_hip_jpeg_encode_into(uint8_t *output, size_t capacity, const uint8_t *data, size_t data_len,
                              const pixo_jpeg_options *options, size_t *out_len)
{
    CallerStorageScope storage(output && capacity);
    PIXO_REQUIRE(options);
    PIXO_REQUIRE(out_len);
    if (capacity) PIXO_REQUIRE(output);
    if (const int rc = checked(*options, true, data_len)) return rc;
    PIXO_REQUIRE(data);
    FileResult r;
    const int rc = encode_host_pixels(data, *options, FileDest::caller(output, capacity), r);
    return deliver_into(rc, r, output, capacity, out_len, /*copy_threads=*/false);
}

int pixo_hip_encode_jpeg(const uint8_t *data, size_t data_len, uint32_t width, uint32_t height,
                         uint8_t color_type, uint8_t quality, uint8_t preset, int subsampling_420,
                         uint8_t **out, size_t *out_len)
{ // wasm.rs:113-142
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    if (color_type != PIXO_GRAY && color_type != PIXO_RGB)
        return fail(PIXO_ERR_INVALID_COLOR_ARG, "Invalid color type for JPEG: " + std::to_string(color_type) +
                                                    ". Expected 0 (Gray) or 2 (Rgb)");
    pixo_jpeg_options o;
    pixo_jpeg_options_from_preset(&o, width, height, quality, preset); // .quality(q).preset(p)
    o.color_type = color_type;                                         // preset keeps the colour type
    o.subsampling = subsampling_420 ? PIXO_S420 : PIXO_S444;           // .subsampling(...) overrides
    return pixo_hip_jpeg_encode(data, data_len, &o, out, out_len);
}

int pixo_hip_coeff_geometry(uint32_t width, uint32_t height, uint8_t color_type, uint8_t subsampling,
                            size_t *y_blocks, size_t *c_blocks)
{
    PIXO_REQUIRE(y_blocks);
    PIXO_REQUIRE(c_blocks);
    if (width == 0 || height == 0)
        return fail(PIXO_ERR_INVALID_DIMENSIONS,
                    "Invalid image dimensions: " + std::to_string(width) + "x" + std::to_string(height));
    if (color_type != PIXO_GRAY && color_type != PIXO_RGB)
        return fail(PIXO_ERR_UNSUPPORTED_COLOR_TYPE, "Unsupported color type for this format");
    const pixo_host::Geometry g = pixo_host::geometry(width, height, color_type, subsampling);
    *y_blocks = g.y_blocks;
    *c_blocks = g.c_blocks;
    return PIXO_OK;
}

int pixo_hip_jpeg_coeffs(const uint8_t *pixels, uint32_t width, uint32_t height, uint8_t color_type,
                         uint8_t subsampling, uint8_t quality, int16_t *y, size_t y_blocks, int16_t *cb,
                         int16_t *cr, size_t c_blocks)
{
    const pixo_jpeg_options o = flat_options(width, height, color_type, subsampling, quality);
    int rc = checked(o);
    if (rc) return rc;
    const pixo_host::Geometry g = geometry_of(o);
    if ((rc = tuple_arrays_checked(g, pixels, y, y_blocks, cb, cr, c_blocks))) return rc;
    const int16_t *hy, *hcb, *hcr;
    if ((rc = coeffs_to_pinned(thread_context(), pixels, o, g, &hy, &hcb, &hcr))) return rc;
    // (the library's copy threads and a huge-page hint for large planes: 50 MB into a caller's fresh arrays)
    big_copy(reinterpret_cast<uint8_t *>(y), reinterpret_cast<const uint8_t *>(hy), g.y_blocks * 128);
    if (g.c_blocks) {
        big_copy(reinterpret_cast<uint8_t *>(cb), reinterpret_cast<const uint8_t *>(hcb), g.c_blocks * 128);
        big_copy(reinterpret_cast<uint8_t *>(cr), reinterpret_cast<const uint8_t *>(hcr), g.c_blocks * 128);
    }
    return PIXO_OK;
}

int pixo_hip_jpeg_coeffs_device(const void *d_pixels, uint32_t width, uint32_t height, uint8_t color_type,
                                uint8_t subsampling, uint8_t quality, uint32_t batch, void *d_y, void *d_cb,
                                void *d_cr, void *stream)
{
    int rc = checked(flat_options(width, height, color_type, subsampling, quality));
    if (rc || (rc = batch_in_range(batch))) return rc;
    PIXO_REQUIRE(d_pixels);
    PIXO_REQUIRE(d_y);
    if (color_type != PIXO_GRAY && (!d_cb || !d_cr)) return fail(PIXO_ERR_COMPRESSION, "Compression error: null argument 'd_cb'/'d_cr'");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const float *qt_all = nullptr;
    if ((rc = device_tables(dev, &qt_all))) return rc;
    const bool gray = color_type == PIXO_GRAY;
    HIP_TRY(pixo_dev::launch_jpeg_coeffs(d_pixels, width, height, gray, !gray && subsampling == PIXO_S420,
                                         batch, d_y, gray ? nullptr : d_cb, gray ? nullptr : d_cr,
                                         qt_all + (quality - 1) * pixo_host::kDeviceQtFloats, static_cast<hipStream_t>(stream)));
    return PIXO_OK;
}

namespace {
int integer_mode_checks(uint32_t width, uint32_t height, uint8_t color_type, uint8_t subsampling, uint8_t quality,
                        pixo_host::QuantTables *qt)
{
    if (const int rc = checked(flat_options(width, height, color_type, subsampling, quality))) return rc;
    if (color_type != PIXO_GRAY && subsampling != PIXO_S444)
        return fail(PIXO_ERR_COMPRESSION, "Compression error: the integer DCT mode is defined per 8x8 block: 4:4:4 or gray only");
    *qt = pixo_host::make_quant_tables(quality);
    return PIXO_OK;
}
} // namespace

int pixo_hip_jpeg_coeffs_integer_device(const void *d_pixels, uint32_t width, uint32_t height, uint8_t color_type,
                                        uint8_t subsampling, uint8_t quality, void *d_y, void *d_cb, void *d_cr, void *stream)
{
    pixo_host::QuantTables qt;
    int rc = integer_mode_checks(width, height, color_type, subsampling, quality, &qt);
    if (rc) return rc;
    PIXO_REQUIRE(d_pixels);
    PIXO_REQUIRE(d_y);
    const bool gray = color_type == PIXO_GRAY;
    if (!gray && (!d_cb || !d_cr)) return fail(PIXO_ERR_COMPRESSION, "Compression error: null argument 'd_cb'/'d_cr'");
    uint16_t ql[64], qc[64];
    for (int i = 0; i < 64; ++i) { ql[i] = static_cast<uint16_t>(qt.lum[i]); qc[i] = static_cast<uint16_t>(qt.chr[i]); } // quantize.rs:56-78
    HIP_TRY(pixo_dev::launch_jpeg_coeffs_integer(d_pixels, width, height, gray, ql, qc, d_y, d_cb, d_cr, static_cast<hipStream_t>(stream)));
    return PIXO_OK;
}

int pixo_hip_jpeg_coeffs_integer(const uint8_t *pixels, uint32_t width, uint32_t height, uint8_t color_type, uint8_t subsampling,
                                 uint8_t quality, int16_t *y, size_t y_blocks, int16_t *cb, int16_t *cr, size_t c_blocks)
{
    pixo_host::QuantTables qt;
    int rc = integer_mode_checks(width, height, color_type, subsampling, quality, &qt);
    if (rc) return rc;
    const pixo_host::Geometry g = pixo_host::geometry(width, height, color_type, PIXO_S444);
    if ((rc = tuple_arrays_checked(g, pixels, y, y_blocks, cb, cr, c_blocks))) return rc;
    Context &c = thread_context();
    if ((rc = c.ensure())) return rc;
    PIXO_ON_DEVICE_OF(c);
    const size_t px_bytes = static_cast<size_t>(width) * height * (g.gray ? 1 : 3), coef_bytes = (g.y_blocks + 2 * g.c_blocks) * 128;
    if ((rc = reserve_pixels(c, px_bytes))) return rc;
    if ((rc = c.d_coef.reserve(coef_bytes))) return rc;
    if ((rc = c.h_coef.reserve(coef_bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(c.d_px.p, pixels, px_bytes, hipMemcpyHostToDevice, c.stream));
    const Planes d = planes_of(c.d_coef.as<int16_t>(), g);
    if ((rc = pixo_hip_jpeg_coeffs_integer_device(c.d_px.p, width, height, color_type, PIXO_S444, quality, d.y, d.cb, d.cr, c.stream))) return rc;
    HIP_TRY(hipMemcpyAsync(c.h_coef.p, c.d_coef.p, coef_bytes, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    const PlanesOf<const int16_t> h = planes_of(c.h_coef.as<const int16_t>(), g);
    std::memcpy(y, h.y, g.y_blocks * 128);
    if (g.c_blocks) {
        std::memcpy(cb, h.cb, g.c_blocks * 128);
        std::memcpy(cr, h.cr, g.c_blocks * 128);
    }
    return PIXO_OK;
}

int pixo_hip_jpeg_entropy_encode(const int16_t *y, const int16_t *cb, const int16_t *cr,
                                 const pixo_jpeg_options *options, uint8_t **out, size_t *out_len)
{
    if (const int rc = tuple_entry_checked(options, out, out_len)) return rc;
    PIXO_REQUIRE(y);
    std::vector<uint8_t> v;
    pixo_host::encode_file(y, cb, cr, *options, v);
    return hand_over(v, out, out_len);
}

int pixo_hip_jpeg_entropy_encode_device(const void *d_y, const void *d_cb, const void *d_cr,
                                        const pixo_jpeg_options *options, uint8_t **out, size_t *out_len)
{
    int rc = tuple_entry_checked(options, out, out_len);
    if (rc) return rc;
    PIXO_REQUIRE(d_y);
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return encode_to_block(*c, FileSource::tuple(d_y, d_cb, d_cr), *options, geometry_of(*options), out, out_len);
}

int pixo_hip_jpeg_encode_device(const void *d_pixels, const pixo_jpeg_options *options, uint8_t **out, size_t *out_len)
{
    PIXO_REQUIRE(options);
    PIXO_REQUIRE(d_pixels);
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    int rc = checked(*options);
    if (rc) return rc;
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return encode_to_block(*c, FileSource::device(d_pixels), *options, geometry_of(*options), out, out_len);
}

int pixo_hip_jpeg_encode_device_into(const void *d_pixels, const pixo_jpeg_options *options, uint8_t *output, size_t capacity,
                                     size_t *out_len)
{
    CallerStorageScope storage(output && capacity);
    PIXO_REQUIRE(options);
    PIXO_REQUIRE(out_len);
    int rc = checked(*options);
    if (rc) return rc;
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    PIXO_REQUIRE(d_pixels); // (behind the context: this entry's own order)
    FileResult r;
    rc = encode_file(*c, FileSource::device(d_pixels), *options, geometry_of(*options), FileDest::caller(output, capacity), r);
    return deliver_into(rc, r, output, capacity, out_len, /*copy_threads=*/true);
}

int pixo_hip_jpeg_encode_batch_device(const void *d_pixels, const pixo_jpeg_options *options, uint32_t batch,
                                      uint8_t **files, size_t *lens)
{
    PIXO_REQUIRE(options);
    PIXO_REQUIRE(files);
    PIXO_REQUIRE(lens);
    int rc = checked(*options);
    if (rc || (rc = batch_in_range(batch))) return rc;
    PIXO_REQUIRE(d_pixels);
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return encode_batch_blocks(*c, d_pixels, *options, geometry_of(*options), batch, files, lens);
}

int pixo_hip_jpeg_encode_batch_device_into(const void *d_pixels, const pixo_jpeg_options *options, uint32_t batch,
                                           uint8_t *arena, size_t capacity, size_t *offsets, size_t *lens)
{
    CallerStorageScope storage(arena && capacity);
    PIXO_REQUIRE(options);
    PIXO_REQUIRE(offsets);
    PIXO_REQUIRE(lens);
    int rc = checked(*options);
    if (rc || (rc = batch_in_range(batch))) return rc;
    PIXO_REQUIRE(d_pixels);
    if (capacity) PIXO_REQUIRE(arena);
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return encode_batch_into(*c, d_pixels, *options, geometry_of(*options), batch, arena, capacity, offsets, lens);
}

uint64_t pixo_hip_debug_lookback_fallbacks(void) { return lookback_fallbacks(); }
uint64_t pixo_hip_debug_routes(int clear) { return take_routes(clear != 0); }
int pixo_hip_debug_dispatch_gate(uint64_t *waits, uint64_t *timeouts)
{
    unsigned long long w = 0, t = 0;
    pixo_dev::dispatch_gate_stats(&w, &t);
    if (waits) *waits = w;
    if (timeouts) *timeouts = t;
    return PIXO_OK;
}

} // extern "C"
