// TEST HARNESS — pixo::convert::layout_images / convert_images / convert_images_device / convert / convert_device of include/pixo.hpp.
//   test_convert_images checks                            the layout and the calls that must throw, none of which touches a device
//   test_convert_images <pixels.bin> <target> <out.bin> <w> <h> <colour type> [<w> <h> <colour type> ...]
//                                                         sources at 16-byte starts in pixels.bin -> the block of converted images
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../include/pixo.hpp"

using pixo::ColorType;
using pixo::convert::Target;

static pixo_png_image image(uint32_t w, uint32_t h, uint8_t ct, uint64_t at)
{
    pixo_png_image im{};
    im.offset = at; im.width = w; im.height = h; im.color_type = ct;
    return im;
}

// which: 0 layout_images, 1 convert_images_device, 2 convert_images
static bool throws(int which, const std::vector<pixo_png_image> &s, const std::vector<pixo_png_image> &d, const void *src, void *dst, size_t len,
                   pixo::Error::Kind kind, const char *what)
{
    try {
        if (which == 0) (void)pixo::convert::layout_images(s, Target::Opaque);
        else if (which == 1) pixo::convert::convert_images_device(src, s, dst, d);
        else (void)pixo::convert::convert_images(static_cast<const uint8_t *>(src), len, s, d);
    } catch (const pixo::Error &e) {
        if (!std::strcmp(e.what(), what) && e.kind() == kind) return true;
        std::printf("threw '%s' (kind %d), expected '%s'\n", e.what(), (int)e.kind(), what);
        return false;
    }
    std::printf("did not throw: %s\n", what);
    return false;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "checks")) {
        uint8_t px[64] = {0}, dst[64];
        const pixo_png_image rgba = image(3, 3, PIXO_RGBA, 0), rgb = image(3, 3, PIXO_RGB, 0), gray = image(3, 3, PIXO_GRAY, 0), empty = image(0, 3, PIXO_RGB, 0),
                             small = image(2, 2, PIXO_RGB, 0);
        bool ok = true;
        // the layout: 5x3 of every colour type; OPAQUE keeps 15, 15, 45, 45 bytes at 0, 16, 32, 80, GRAY 15 bytes each
        size_t total = 0;
        const std::vector<pixo_png_image> four = {image(5, 3, PIXO_GRAY, 7), image(5, 3, PIXO_GRAY_ALPHA, 7), image(5, 3, PIXO_RGB, 7), image(5, 3, PIXO_RGBA, 7)};
        const std::vector<pixo_png_image> opaque = pixo::convert::layout_images(four, Target::Opaque, &total);
        ok = opaque.size() == 4 && opaque[0].color_type == PIXO_GRAY && opaque[1].color_type == PIXO_GRAY && opaque[2].color_type == PIXO_RGB &&
             opaque[3].color_type == PIXO_RGB && opaque[1].offset == 16 && opaque[2].offset == 32 && opaque[3].offset == 80 && total == 125 &&
             opaque[3].width == 5 && opaque[3].height == 3 && ok;
        const std::vector<pixo_png_image> grays = pixo::convert::layout_images(four, Target::Gray, &total);
        ok = grays.size() == 4 && grays[3].color_type == PIXO_GRAY && grays[3].offset == 48 && total == 63 && ok;
        if (!ok) std::puts("layout_images: records differ");
        // (an empty vector has no array: the ABI's first check answers)
        for (int which = 0; which < 3; ++which)
            ok = throws(which, {}, {}, px, dst, 64, pixo::Error::Kind::CompressionError, "Compression error: null argument 'src_images'") && ok;
        ok = throws(0, {rgba, empty}, {}, px, dst, 64, pixo::Error::Kind::InvalidDimensions, "Invalid image dimensions: 0x3 (image 1)") && ok;
        for (int which = 1; which < 3; ++which) {
            ok = throws(which, {rgba, rgba, empty}, {rgb, rgb, rgb}, px, dst, 64, pixo::Error::Kind::InvalidDimensions,
                        "Invalid image dimensions: 0x3 (image 2)") && ok;
            ok = throws(which, {rgba, rgba}, {rgb, small}, px, dst, 64, pixo::Error::Kind::CompressionError, "Compression error: sizes differ (image 1)") && ok;
            ok = throws(which, {rgba, gray}, {rgb, rgb}, px, dst, 64, pixo::Error::Kind::UnsupportedColorType,
                        "Unsupported color type for this format (image 1)") && ok;
        }
        ok = throws(1, {rgba}, {rgb}, nullptr, dst, 0, pixo::Error::Kind::CompressionError, "Compression error: null argument 'd_src'") && ok;
        ok = throws(1, {rgba}, {rgb}, px, nullptr, 0, pixo::Error::Kind::CompressionError, "Compression error: null argument 'd_dst'") && ok;
        ok = throws(2, {rgba}, {rgb}, px, dst, 35, pixo::Error::Kind::InvalidDataLength, "Invalid pixel data length: expected 36 bytes, got 35") && ok;
        try { // the single entries
            (void)pixo::convert::convert(px, 9, 3, 3, ColorType::Gray, ColorType::Rgb);
            ok = false;
            std::puts("did not throw: Gray -> Rgb");
        } catch (const pixo::Error &e) {
            ok = e.kind() == pixo::Error::Kind::UnsupportedColorType && !std::strcmp(e.what(), "Unsupported color type for this format") && ok;
        }
        try {
            pixo::convert::convert_device(nullptr, 3, 3, ColorType::Rgba, ColorType::Rgb, dst);
            ok = false;
            std::puts("did not throw: a null d_src");
        } catch (const pixo::Error &e) {
            ok = !std::strcmp(e.what(), "Compression error: null argument 'd_src'") && ok;
        }
        try { // the mirror's own check
            pixo::convert::convert_images_device(px, {rgba, rgba}, dst, {rgb});
            ok = false;
            std::puts("did not throw: one destination for two sources");
        } catch (const std::invalid_argument &) {
        }
        if (ok) std::puts("all checks passed");
        return ok ? 0 : 1;
    }
    if (argc < 7 || (argc - 4) % 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> px((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<pixo_png_image> sources;
    uint64_t at = 0;
    for (int k = 4; k < argc; k += 3) {
        const uint32_t w = (uint32_t)std::atoi(argv[k]), h = (uint32_t)std::atoi(argv[k + 1]);
        const uint8_t ct = (uint8_t)std::atoi(argv[k + 2]);
        sources.push_back(image(w, h, ct, at));
        at = (at + (uint64_t)w * h * (ct + 1u) + 15) & ~uint64_t{15};
    }
    size_t total = 0;
    const std::vector<pixo_png_image> laid = pixo::convert::layout_images(sources, (Target)std::atoi(argv[2]), &total);
    const std::vector<uint8_t> out = pixo::convert::convert_images(px.data(), px.size(), sources, laid);
    if (out.size() != total) return 1;
    // the first image once more through the single entry
    const pixo_png_image &a = sources[0], &b = laid[0];
    const std::vector<uint8_t> one = pixo::convert::convert(px.data(), (size_t)a.width * a.height * (a.color_type + 1u), a.width, a.height,
                                                            (ColorType)a.color_type, (ColorType)b.color_type);
    if (one.size() != (size_t)b.width * b.height * (b.color_type + 1u) || std::memcmp(one.data(), out.data(), one.size())) return 1;
    std::ofstream(argv[3], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), (std::streamsize)out.size());
    std::puts("all checks passed");
    return 0;
}
