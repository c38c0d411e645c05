// TEST HARNESS — pixo::decode::decode_jpeg_batch and decode_jpeg_batch_device of include/pixo.hpp with device_entropy = true.
//   test_jpeg_decode_entropy checks                            refusals that touch no device, with the flag
//   test_jpeg_decode_entropy <out.bin> <one_thread 0|1> <file.jpg> [<file.jpg> ...]
//                                                              the images' pixels back to back in out.bin, one line
//                                                              "width height color_type bytes" per image on stdout
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../include/pixo.hpp"

static bool throws(const std::vector<pixo_png_file> &files, bool one_thread, pixo::Error::Kind kind, const char *what)
{
    try {
        (void)pixo::decode::decode_jpeg_batch(files, one_thread, true);
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
        static_assert(PIXO_DECODE_DEVICE_ENTROPY == 4u && PIXO_DECODE_DEVICE_INFLATE == 2u && PIXO_DECODE_ONE_THREAD == 1u, "the flags' bits");
        const uint8_t junk[12] = {'n', 'o', 't', 'h', 'i', 'n', 'g', 0, 0, 0, 0, 0};
        const pixo_png_file not_jpeg{junk, sizeof junk}, nowhere{nullptr, 4};
        bool ok = true;
        for (int one_thread = 0; one_thread < 2; ++one_thread) {
            ok = throws({}, one_thread, pixo::Error::Kind::CompressionError, "Compression error: null argument 'files'") && ok;
            ok = throws({not_jpeg}, one_thread, pixo::Error::Kind::InvalidDecode, "Decode error: not a JPEG file (image 0)") && ok;
            ok = throws({nowhere, not_jpeg}, one_thread, pixo::Error::Kind::CompressionError, "Compression error: null argument 'data' (image 0)") && ok;
        }
        uint32_t sub = 0, group = 0, cap = 0, least = 0;
        pixo_hip_jpeg_entropy_geometry(&sub, &group, &cap, &least);
        ok = sub && group && cap && least && ok;
        if (ok) std::puts("all checks passed");
        return ok ? 0 : 1;
    }
    if (argc < 4) return 2;
    std::vector<std::vector<uint8_t>> held;
    std::vector<pixo_png_file> files;
    for (int k = 3; k < argc; ++k) {
        std::ifstream in(argv[k], std::ios::binary);
        held.emplace_back((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    }
    for (const std::vector<uint8_t> &f : held) files.push_back({f.data(), f.size()});
    const bool one_thread = argv[2][0] == '1';
    const std::vector<pixo::decode::JpegImage> images = pixo::decode::decode_jpeg_batch(files, one_thread, true);
    const std::vector<pixo::decode::JpegImage> plain = pixo::decode::decode_jpeg_batch(files, one_thread);
    if (images.size() != files.size() || plain.size() != files.size()) return 1;
    for (size_t i = 0; i < images.size(); ++i)
        if (images[i].width != plain[i].width || images[i].height != plain[i].height || images[i].color_type != plain[i].color_type || images[i].pixels != plain[i].pixels) {
            std::printf("image %zu differs from the one without the flag\n", i);
            return 1;
        }
    std::ofstream out(argv[1], std::ios::binary);
    for (const pixo::decode::JpegImage &im : images) {
        std::printf("%u %u %d %zu\n", im.width, im.height, (int)im.color_type, im.pixels.size());
        out.write(reinterpret_cast<const char *>(im.pixels.data()), (std::streamsize)im.pixels.size());
    }
    std::puts("all checks passed");
    return 0;
}
