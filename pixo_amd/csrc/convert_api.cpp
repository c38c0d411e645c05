// convert_api.cpp — the extern "C" colour-conversion entry points: what the reference's front end does between a decode and
// an encode (src/bin/pixo.rs:478-513, 619-638), on pixels that stay in HBM.  The layout a target gives a batch, the checks in
// the order include/pixo_hip.h documents, the plan (kind, form and tiles per image, sub-batches whose launches stay within
// their tiles), the records of the flat launches (convert_math.h), one launch per class of images present (convert.hip).
// The steps every batch driver takes, and their order: DESIGN.md §4.0; the shared ones: batch_steps.hpp.
#include "batch_steps.hpp"
#include "convert.hpp"

#include <algorithm>
#include <string>
#include <vector>

using namespace pixo_capi;
namespace cv = pixo_convert;

namespace {

// A zero side, a side above 2^24 (the resize entries' limit, which bounds an image at 2^50 bytes)
int check_sides(uint32_t w, uint32_t h, const std::string &where)
{
    int rc = PIXO_OK;
    if (w == 0 || h == 0) rc = bad_dimensions(w, h);
    else if (w > cv::kMaxSide || h > cv::kMaxSide) rc = too_large(w, h, cv::kMaxSide);
    return rc && !where.empty() ? fail(rc, t_error + where) : rc;
}
uint32_t image_tiles_cap() { return debug().convert_images_tiles ? debug().convert_images_tiles : cv::kImageTiles; }
uint64_t launch_tiles_cap() { return debug().convert_images_tiles ? 2ull * debug().convert_images_tiles : cv::kMaxTiles; }

// The checks the images entries share, in their order.  *src_end / *dst_end: the furthest image's end.
int convert_images_checks(const pixo_png_image *src_images, const pixo_png_image *dst_images, uint32_t batch, uint64_t *src_end, uint64_t *dst_end)
{
    PIXO_REQUIRE(src_images);
    PIXO_REQUIRE(dst_images);
    int rc = batch_in_range(batch);
    if (rc) return rc;
    *src_end = *dst_end = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        const std::string here = where(i);
        const pixo_png_image &a = src_images[i], &b = dst_images[i];
        if ((rc = check_sides(a.width, a.height, here)) || (rc = check_sides(b.width, b.height, here))) return rc;
        if (a.color_type > PIXO_RGBA) return bad_color_type(a.color_type, here);
        if (b.color_type > PIXO_RGBA) return bad_color_type(b.color_type, here);
        if (a.width != b.width || a.height != b.height) return fail(PIXO_ERR_COMPRESSION, "Compression error: sizes differ" + here);
        if (cv::kind_of(a.color_type, b.color_type) == cv::K_NONE)
            return fail(PIXO_ERR_UNSUPPORTED_COLOR_TYPE, "Unsupported color type for this format" + here);
        if ((rc = record_extent(a.offset, image_bytes(a), "input", here, src_end)) || (rc = record_extent(b.offset, image_bytes(b), "output", here, dst_end)))
            return rc;
    }
    return PIXO_OK;
}

// What the driver decided for the images, before anything touches a device (also: pixo_hip_debug_convert_images_plan).
struct ImagesPlan {
    SubBatches sub_first;
    std::vector<uint8_t> kind, form; // per image
    std::vector<uint32_t> tiles;     // per image: its workgroups
    uint32_t launches = 0;           // summed over the sub-batches: one per class present in each
};
// The images have passed convert_images_checks; src_base / dst_base: the blocks' addresses (the plan entry: their residues).
void convert_images_plan(const pixo_png_image *src, const pixo_png_image *dst, uint32_t batch, uint64_t src_base, uint64_t dst_base, ImagesPlan &p)
{
    const uint32_t cap = image_tiles_cap();
    const uint64_t limit = launch_tiles_cap();
    p.kind.assign(batch, 0);
    p.form.assign(batch, 0);
    p.tiles.assign(batch, 0);
    uint64_t held[cv::kClasses] = {}; // the current sub-batch's tiles so far, by class
    for (uint32_t i = 0; i < batch; ++i) {
        const int kind = cv::kind_of(src[i].color_type, dst[i].color_type), form = cv::form_of(src_base + src[i].offset, dst_base + dst[i].offset);
        const uint32_t c = cv::class_of(kind, form), t = cv::tiles_of(static_cast<uint64_t>(src[i].width) * src[i].height, cap);
        // (one image's tiles stay within a launch: tiles_of)
        if (p.sub_first.starts_at(i, held[c] + t > limit)) std::fill(held, held + cv::kClasses, uint64_t{0});
        if (held[c] == 0) p.launches += 1;
        held[c] += t;
        p.kind[i] = static_cast<uint8_t>(kind);
        p.form[i] = static_cast<uint8_t>(form);
        p.tiles[i] = t;
    }
    p.sub_first.close(batch);
}

// Enqueues the images on `s`: d_src + src[i].offset -> d_dst + dst[i].offset.  The records of all sub-batches are built in the
// pinned staging; every sub-batch's go up in one copy, its launches behind it.
int convert_images_on_device(Context &c, const uint8_t *d_src, const pixo_png_image *src, uint8_t *d_dst, const pixo_png_image *dst, uint32_t batch,
                             hipStream_t s)
{
    ImagesPlan p;
    convert_images_plan(src, dst, batch, reinterpret_cast<uint64_t>(d_src), reinterpret_cast<uint64_t>(d_dst), p);
    int rc = await_last_job(c.cv_done); // (it reads cv_records, which go up from h_cv_records)
    if (rc) return rc;
    // everything is reserved before any address is handed out (a growing reserve frees first)
    const size_t up_bytes = static_cast<size_t>(batch) * sizeof(cv::Record);
    if ((rc = c.h_cv_records.reserve(up_bytes)) || (rc = c.cv_records.reserve(up_bytes))) return rc;
    cv::Record *stage = c.h_cv_records.as<cv::Record>();
    const cv::Record *d_records = c.cv_records.as<cv::Record>();
    std::vector<cv::Item> items;
    std::vector<cv::Record> table;
    std::vector<cv::Launch> launches;
    std::vector<uint32_t> record_item;
    for (size_t k = 0; k + 1 < p.sub_first.size(); ++k) {
        const uint32_t first = p.sub_first[k], n = p.sub_first[k + 1] - first;
        items.clear();
        for (uint32_t i = first; i < first + n; ++i)
            items.push_back(cv::Item{reinterpret_cast<uint64_t>(d_src) + src[i].offset, reinterpret_cast<uint64_t>(d_dst) + dst[i].offset,
                                     static_cast<uint64_t>(src[i].width) * src[i].height, p.kind[i], bytes_per_pixel(src[i].color_type)});
        if (!cv::build_table(items, image_tiles_cap(), launch_tiles_cap(), table, launches, record_item))
            return fail(PIXO_ERR_COMPRESSION, "Compression error: convert launch too large"); // (the plan cuts before that)
        std::copy(table.begin(), table.end(), stage + first);
        HIP_TRY(hipMemcpyAsync(c.cv_records.as<cv::Record>() + first, stage + first, n * sizeof(cv::Record), hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(c.cv_done, s)); // (until the job's own record: the uploads so far)
        for (const cv::Launch &l : launches)
            HIP_TRY(pixo_dev::launch_convert_images(d_records + first + l.first_record, l.count, l.tiles, static_cast<int>(l.cls / cv::kForms),
                                                    static_cast<int>(l.cls % cv::kForms), s));
    }
    HIP_TRY(hipEventRecord(c.cv_done, s));
    return PIXO_OK;
}

// The single entries' checks, in their order
int convert_checks(uint32_t width, uint32_t height, uint8_t src_ct, uint8_t dst_ct, int *kind)
{
    int rc = check_sides(width, height, "");
    if (rc) return rc;
    if (src_ct > PIXO_RGBA) return bad_color_type(src_ct, "");
    if (dst_ct > PIXO_RGBA) return bad_color_type(dst_ct, "");
    if ((*kind = cv::kind_of(src_ct, dst_ct)) == cv::K_NONE) return fail(PIXO_ERR_UNSUPPORTED_COLOR_TYPE, "Unsupported color type for this format");
    return PIXO_OK;
}
int convert_on_device(const uint8_t *d_src, uint32_t width, uint32_t height, uint8_t src_ct, int kind, uint8_t *d_dst, hipStream_t s)
{
    const uint64_t pixels = static_cast<uint64_t>(width) * height;
    HIP_TRY(pixo_dev::launch_convert(d_src, d_dst, pixels, bytes_per_pixel(src_ct), kind,
                                     cv::form_of(reinterpret_cast<uint64_t>(d_src), reinterpret_cast<uint64_t>(d_dst)),
                                     cv::tiles_of(pixels, image_tiles_cap()), s));
    return PIXO_OK;
}

} // namespace

extern "C" {

int pixo_hip_convert_images_layout(const pixo_png_image *src_images, uint32_t batch, uint8_t target, pixo_png_image *dst_images, size_t *total)
{
    PIXO_REQUIRE(src_images);
    PIXO_REQUIRE(dst_images);
    PIXO_REQUIRE(total);
    int rc = batch_in_range(batch);
    if (rc) return rc;
    if (cv::target_type(target, 0) < 0) return fail(PIXO_ERR_COMPRESSION, "Compression error: unknown convert target " + std::to_string(target));
    for (uint32_t i = 0; i < batch; ++i) { // nothing is written before every image has passed
        const pixo_png_image &a = src_images[i];
        if ((rc = check_sides(a.width, a.height, where(i)))) return rc;
        if (a.color_type > PIXO_RGBA) return bad_color_type(a.color_type, where(i));
    }
    uint64_t at = 0, end = 0;
    std::vector<pixo_png_image> laid(batch); // (dst_images may be src_images)
    for (uint32_t i = 0; i < batch; ++i) {
        const pixo_png_image &a = src_images[i]; // (at <= 2^62 + 15, an image at most 2^50 bytes: no wrap)
        laid[i] = lay_out(at, a.width, a.height, static_cast<uint8_t>(cv::target_type(target, a.color_type)), &end);
        if (end > (uint64_t{1} << 62)) return fail(PIXO_ERR_COMPRESSION, "Compression error: batch output too large");
    }
    report(laid, dst_images);
    *total = static_cast<size_t>(end);
    return PIXO_OK;
}

int pixo_hip_convert_images_device(const void *d_src, const pixo_png_image *src_images, void *d_dst, const pixo_png_image *dst_images, uint32_t batch,
                                   void *stream)
{
    uint64_t src_end = 0, dst_end = 0;
    int rc = convert_images_checks(src_images, dst_images, batch, &src_end, &dst_end);
    if (rc) return rc;
    PIXO_REQUIRE(d_src);
    PIXO_REQUIRE(d_dst);
    PIXO_CALLER_STREAM_CONTEXT(c, s, stream);
    return convert_images_on_device(*c, static_cast<const uint8_t *>(d_src), src_images, static_cast<uint8_t *>(d_dst), dst_images, batch, s);
}

int pixo_hip_convert_images(const uint8_t *data, size_t data_len, const pixo_png_image *src_images, const pixo_png_image *dst_images, uint32_t batch,
                            uint8_t **out, size_t *out_len)
{
    uint64_t src_end = 0, dst_end = 0;
    int rc = convert_images_checks(src_images, dst_images, batch, &src_end, &dst_end);
    if (rc) return rc;
    PIXO_REQUIRE(data);
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    if (data_len < src_end) return bad_length(static_cast<size_t>(src_end), data_len);
    PIXO_THREAD_CONTEXT(c);
    if ((rc = upload(c, c.cv_in, data, static_cast<size_t>(src_end))) || (rc = reserve16(c.cv_out, static_cast<size_t>(dst_end)))) return rc;
    uint8_t *block = alloc_file(static_cast<size_t>(dst_end));
    if (!block) return fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
    rc = convert_images_on_device(c, c.cv_in.as<uint8_t>(), src_images, c.cv_out.as<uint8_t>(), dst_images, batch, c.stream);
    return download_block(c, rc, block, c.cv_out.p, static_cast<size_t>(dst_end), out, out_len);
}

int pixo_hip_convert_device(const void *d_src, uint32_t width, uint32_t height, uint8_t src_color_type, uint8_t dst_color_type, void *d_dst, void *stream)
{
    int kind = cv::K_NONE;
    int rc = convert_checks(width, height, src_color_type, dst_color_type, &kind);
    if (rc) return rc;
    PIXO_REQUIRE(d_src);
    PIXO_REQUIRE(d_dst);
    PIXO_CALLER_STREAM_CONTEXT(c, s, stream);
    return convert_on_device(static_cast<const uint8_t *>(d_src), width, height, src_color_type, kind, static_cast<uint8_t *>(d_dst), s);
}

int pixo_hip_convert(const uint8_t *data, size_t data_len, uint32_t width, uint32_t height, uint8_t src_color_type, uint8_t dst_color_type, uint8_t **out,
                     size_t *out_len)
{
    int kind = cv::K_NONE;
    int rc = convert_checks(width, height, src_color_type, dst_color_type, &kind);
    if (rc) return rc;
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    const size_t pixels = static_cast<size_t>(width) * height;
    const size_t in_bytes = pixels * bytes_per_pixel(src_color_type), out_bytes = pixels * bytes_per_pixel(dst_color_type);
    if (data_len != in_bytes) return bad_length(in_bytes, data_len);
    PIXO_REQUIRE(data);
    PIXO_THREAD_CONTEXT(c);
    if ((rc = upload(c, c.cv_in, data, in_bytes)) || (rc = reserve16(c.cv_out, out_bytes))) return rc;
    uint8_t *block = alloc_file(out_bytes);
    if (!block) return fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
    rc = convert_on_device(c.cv_in.as<uint8_t>(), width, height, src_color_type, kind, c.cv_out.as<uint8_t>(), c.stream);
    return download_block(c, rc, block, c.cv_out.p, out_bytes, out, out_len);
}

int pixo_hip_debug_convert_images_plan(const pixo_png_image *src_images, const pixo_png_image *dst_images, uint32_t batch, uint32_t src_align,
                                       uint32_t dst_align, uint32_t *sub_first, uint32_t *sub_count, uint8_t *kind, uint8_t *form, uint32_t *tiles,
                                       uint32_t *launches)
{
    uint64_t src_end = 0, dst_end = 0;
    int rc = convert_images_checks(src_images, dst_images, batch, &src_end, &dst_end);
    if (rc) return rc;
    PIXO_REQUIRE(sub_first);
    PIXO_REQUIRE(sub_count);
    PIXO_REQUIRE(kind);
    PIXO_REQUIRE(form);
    PIXO_REQUIRE(tiles);
    PIXO_REQUIRE(launches);
    ImagesPlan p;
    convert_images_plan(src_images, dst_images, batch, src_align & 15u, dst_align & 15u, p);
    p.sub_first.report(sub_first, sub_count);
    std::copy(p.kind.begin(), p.kind.end(), kind);
    std::copy(p.form.begin(), p.form.end(), form);
    std::copy(p.tiles.begin(), p.tiles.end(), tiles);
    *launches = p.launches;
    return PIXO_OK;
}

uint32_t pixo_hip_debug_convert_tile_pixels(void) { return cv::kTilePixels; }

} // extern "C"
