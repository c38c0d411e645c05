// TEST HARNESS — pixo::resize::fit_images / resize_images / resize_images_device of include/pixo.hpp.
//   test_resize_images checks                                  the sizes and the calls that must throw, none of which touches a device
//   test_resize_images <pixels.bin> <box_w> <box_h> <algorithm> <out.bin> <w> <h> <colour type> [<w> <h> <colour type> ...]
//                                                              sources at 16-byte starts in pixels.bin -> the block of fitted images
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../include/pixo.hpp"

using pixo::resize::ResizeAlgorithm;

static pixo_png_image image(uint32_t w, uint32_t h, uint8_t ct, uint64_t at)
{
    pixo_png_image im{};
    im.offset = at; im.width = w; im.height = h; im.color_type = ct;
    return im;
}

// which: 0 fit_images, 1 resize_images_device, 2 resize_images
static bool throws(int which, const std::vector<pixo_png_image> &s, const std::vector<pixo_png_image> &d, const void *src, void *dst, size_t len,
                   pixo::Error::Kind kind, const char *what)
{
    try {
        if (which == 0) (void)pixo::resize::fit_images(s, 4, 4);
        else if (which == 1) pixo::resize::resize_images_device(src, s, dst, d, ResizeAlgorithm::Lanczos3);
        else (void)pixo::resize::resize_images(static_cast<const uint8_t *>(src), len, s, d, ResizeAlgorithm::Lanczos3);
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
        static_assert(sizeof(pixo_png_image) == 24, "the ABI's image record");
        uint8_t px[64] = {0}, dst[64];
        const pixo_png_image good = image(3, 3, PIXO_RGB, 0), small = image(2, 2, PIXO_RGB, 0), empty = image(0, 3, PIXO_RGB, 0),
                             gray = image(2, 2, PIXO_GRAY, 16);
        bool ok = true;
        // the sizes: 30x10 and 10x30 into 20x20, the layout of a decode batch
        size_t total = 0;
        const std::vector<pixo_png_image> fitted = pixo::resize::fit_images({image(30, 10, PIXO_RGBA, 0), image(10, 30, PIXO_GRAY, 1200)}, 20, 20, false, &total);
        ok = fitted.size() == 2 && fitted[0].width == 20 && fitted[0].height == 7 && fitted[0].color_type == PIXO_RGBA && fitted[0].offset == 0 &&
             fitted[1].width == 7 && fitted[1].height == 20 && fitted[1].color_type == PIXO_GRAY && fitted[1].offset == 560 && total == 700 && ok;
        const std::vector<pixo_png_image> kept = pixo::resize::fit_images({image(3, 2, PIXO_RGB, 0)}, 20, 20, true);
        ok = kept.size() == 1 && kept[0].width == 3 && kept[0].height == 2 && ok;
        if (!ok) std::puts("fit_images: sizes differ");
        // (an empty vector has no array: the ABI's first check answers)
        for (int which = 0; which < 3; ++which)
            ok = throws(which, {}, {}, px, dst, 64, pixo::Error::Kind::CompressionError, "Compression error: null argument 'src_images'") && ok;
        ok = throws(0, {good, empty}, {}, px, dst, 64, pixo::Error::Kind::InvalidDimensions, "Invalid image dimensions: 0x3 (image 1)") && ok;
        for (int which = 1; which < 3; ++which) {
            ok = throws(which, {good, good, empty}, {small, small, small}, px, dst, 64, pixo::Error::Kind::InvalidDimensions,
                        "Invalid image dimensions: 0x3 (image 2)") && ok;
            ok = throws(which, {good, good}, {small, gray}, px, dst, 64, pixo::Error::Kind::CompressionError,
                        "Compression error: colour types differ (image 1)") && ok;
            ok = throws(which, {good, image(1u << 25, 1, PIXO_RGB, 0)}, {small, small}, px, dst, 64, pixo::Error::Kind::ImageTooLarge,
                        "Image 33554432x2 exceeds maximum dimension 16777216 (image 1)") && ok;
        }
        ok = throws(1, {good}, {small}, nullptr, dst, 0, pixo::Error::Kind::CompressionError, "Compression error: null argument 'd_src'") && ok;
        ok = throws(1, {good}, {small}, px, nullptr, 0, pixo::Error::Kind::CompressionError, "Compression error: null argument 'd_dst'") && ok;
        ok = throws(2, {good}, {small}, px, dst, 26, pixo::Error::Kind::InvalidDataLength, "Invalid pixel data length: expected 27 bytes, got 26") && ok;
        try { // the mirror's own check
            pixo::resize::resize_images_device(px, {good, good}, dst, {small}, ResizeAlgorithm::Nearest);
            ok = false;
            std::puts("did not throw: one destination for two sources");
        } catch (const std::invalid_argument &) {
        }
        if (ok) std::puts("all checks passed");
        return ok ? 0 : 1;
    }
    if (argc < 9 || (argc - 6) % 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> px((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const uint32_t box_w = (uint32_t)std::atoi(argv[2]), box_h = (uint32_t)std::atoi(argv[3]);
    std::vector<pixo_png_image> sources;
    uint64_t at = 0;
    for (int k = 6; k < argc; k += 3) {
        const uint32_t w = (uint32_t)std::atoi(argv[k]), h = (uint32_t)std::atoi(argv[k + 1]);
        const uint8_t ct = (uint8_t)std::atoi(argv[k + 2]);
        sources.push_back(image(w, h, ct, at));
        at = (at + (uint64_t)w * h * (ct + 1u) + 15) & ~uint64_t{15};
    }
    size_t total = 0;
    const std::vector<pixo_png_image> fitted = pixo::resize::fit_images(sources, box_w, box_h, false, &total);
    const std::vector<uint8_t> out = pixo::resize::resize_images(px.data(), px.size(), sources, fitted, (ResizeAlgorithm)std::atoi(argv[4]));
    if (out.size() != total) return 1;
    std::ofstream(argv[5], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), (std::streamsize)out.size());
    std::puts("all checks passed");
    return 0;
}
