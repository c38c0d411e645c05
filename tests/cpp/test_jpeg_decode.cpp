// TEST HARNESS — pixo::decode::decode_jpeg and decode_jpeg_batch of include/pixo.hpp.
//   test_jpeg_decode checks                                    the calls that must throw, none of which touches a device
//   test_jpeg_decode <out.bin> <file.jpg> [<file.jpg> ...]     every file through decode_jpeg and all through decode_jpeg_batch
//                                                              (the two must agree); the images' pixels back to back in
//                                                              out.bin, one line "width height color_type bytes" per image
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../include/pixo.hpp"

template <class F> static bool throws(F &&call, pixo::Error::Kind kind, const char *what)
{
    try {
        call();
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
        const std::vector<uint8_t> junk = {'n', 'o', 't', 'h', 'i', 'n', 'g'};
        const std::vector<uint8_t> progressive = {0xFF, 0xD8, 0xFF, 0xC2, 0x00, 0x02};
        const std::vector<uint8_t> empty = {0xFF, 0xD8, 0xFF, 0xD9};
        const pixo_png_file f_junk{junk.data(), junk.size()}, f_prog{progressive.data(), progressive.size()}, nowhere{nullptr, 4};
        bool ok = true;
        ok = throws([&] { (void)pixo::decode::decode_jpeg(junk); }, pixo::Error::Kind::InvalidDecode, "Decode error: not a JPEG file") && ok;
        ok = throws([&] { (void)pixo::decode::decode_jpeg(progressive); }, pixo::Error::Kind::UnsupportedDecode, "Unsupported: progressive JPEG not supported") && ok;
        ok = throws([&] { (void)pixo::decode::decode_jpeg(empty); }, pixo::Error::Kind::InvalidDecode, "Decode error: no image data found") && ok;
        for (int one_thread = 0; one_thread < 2; ++one_thread) {
            ok = throws([&] { (void)pixo::decode::decode_jpeg_batch({}, one_thread); }, pixo::Error::Kind::CompressionError, "Compression error: null argument 'files'") && ok;
            ok = throws([&] { (void)pixo::decode::decode_jpeg_batch({f_prog, f_junk}, one_thread); }, pixo::Error::Kind::UnsupportedDecode,
                        "Unsupported: progressive JPEG not supported (image 0)") && ok;
            ok = throws([&] { (void)pixo::decode::decode_jpeg_batch({nowhere, f_junk}, one_thread); }, pixo::Error::Kind::CompressionError,
                        "Compression error: null argument 'data' (image 0)") && ok;
        }
        ok = throws([&] { (void)pixo::decode::decode_jpeg_batch_device({f_junk}, nullptr, 0); }, pixo::Error::Kind::InvalidDecode,
                    "Decode error: not a JPEG file (image 0)") && ok;
        if (ok) std::puts("all checks passed");
        return ok ? 0 : 1;
    }
    if (argc < 3) return 2;
    std::vector<std::vector<uint8_t>> held;
    std::vector<pixo_png_file> files;
    for (int k = 2; k < argc; ++k) {
        std::ifstream in(argv[k], std::ios::binary);
        held.emplace_back((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    }
    for (const std::vector<uint8_t> &f : held) files.push_back({f.data(), f.size()});
    const std::vector<pixo::decode::JpegImage> images = pixo::decode::decode_jpeg_batch(files);
    if (images.size() != files.size()) return 1;
    std::ofstream out(argv[1], std::ios::binary);
    for (size_t i = 0; i < images.size(); ++i) {
        const pixo::decode::JpegImage &im = images[i];
        const pixo::decode::JpegImage one = pixo::decode::decode_jpeg(held[i]);
        if (one.pixels != im.pixels || one.width != im.width || one.height != im.height || one.color_type != im.color_type) {
            std::printf("image %zu: decode_jpeg and decode_jpeg_batch differ\n", i);
            return 1;
        }
        std::printf("%u %u %d %zu\n", im.width, im.height, (int)im.color_type, im.pixels.size());
        out.write(reinterpret_cast<const char *>(im.pixels.data()), (std::streamsize)im.pixels.size());
    }
    std::puts("all checks passed");
    return 0;
}
