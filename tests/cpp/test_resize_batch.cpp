// TEST HARNESS — pixo::resize::resize_batch / resize_batch_device of include/pixo.hpp.
//   test_resize_batch checks                                   the calls that must throw, none of which touches a device
//   test_resize_batch <pixels.bin> <dw> <dh> <algorithm> <out.bin> <w> <h> [<w> <h> ...]
//                                                              RGB sources back to back in pixels.bin -> the block of images
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../include/pixo.hpp"

using pixo::ColorType;
using pixo::resize::ResizeAlgorithm;

static bool throws(bool device, const std::vector<pixo_resize_source> &s, uint32_t dw, uint32_t dh, void *dst, pixo::Error::Kind kind, const char *what)
{
    try {
        if (device) pixo::resize::resize_batch_device(s, dw, dh, ColorType::Rgb, ResizeAlgorithm::Lanczos3, dst);
        else (void)pixo::resize::resize_batch(s, dw, dh, ColorType::Rgb, ResizeAlgorithm::Lanczos3);
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
        static_assert(sizeof(pixo_resize_source) == 16, "the ABI's source entry");
        uint8_t px[27] = {0}, dst[4];
        const pixo_resize_source good{px, 3, 3}, empty{px, 0, 3}, nowhere{nullptr, 3, 3};
        bool ok = true;
        for (int device = 0; device < 2; ++device) {
            // (an empty vector has no array: the ABI's first check answers)
            ok = throws(device, {}, 4, 4, dst, pixo::Error::Kind::CompressionError, "Compression error: null argument 'sources'") && ok;
            ok = throws(device, {good, good, empty}, 4, 4, dst, pixo::Error::Kind::InvalidDimensions, "Invalid image dimensions: 0x3 (image 2)") && ok;
            ok = throws(device, {good, good}, 4, 0, dst, pixo::Error::Kind::InvalidDimensions, "Invalid image dimensions: 4x0 (image 0)") && ok;
            ok = throws(device, {good, {px, 1u << 25, 1}}, 4, 4, dst, pixo::Error::Kind::ImageTooLarge,
                        "Image 33554432x4 exceeds maximum dimension 16777216 (image 1)") && ok;
            ok = throws(device, {good, nowhere}, 4, 4, dst, pixo::Error::Kind::CompressionError, "Compression error: null argument 'pixels' (image 1)") && ok;
        }
        ok = throws(true, {good}, 4, 4, nullptr, pixo::Error::Kind::CompressionError, "Compression error: null argument 'd_dst'") && ok;
        if (ok) std::puts("all checks passed");
        return ok ? 0 : 1;
    }
    if (argc < 8 || (argc - 6) % 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> px((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const uint32_t dw = (uint32_t)std::atoi(argv[2]), dh = (uint32_t)std::atoi(argv[3]);
    std::vector<pixo_resize_source> sources;
    size_t at = 0;
    for (int k = 6; k < argc; k += 2) {
        const uint32_t w = (uint32_t)std::atoi(argv[k]), h = (uint32_t)std::atoi(argv[k + 1]);
        sources.push_back({px.data() + at, w, h});
        at += (size_t)w * h * 3;
    }
    if (at != px.size()) return 3;
    const std::vector<uint8_t> out = pixo::resize::resize_batch(sources, dw, dh, ColorType::Rgb, (ResizeAlgorithm)std::atoi(argv[4]));
    if (out.size() != sources.size() * dw * dh * 3) return 1;
    std::ofstream(argv[5], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), (std::streamsize)out.size());
    std::puts("all checks passed");
    return 0;
}
