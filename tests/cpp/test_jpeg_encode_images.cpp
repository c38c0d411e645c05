// TEST HARNESS — pixo::jpeg::encode_images / encode_images_device of include/pixo.hpp.
//   test_jpeg_encode_images checks                    the calls that must throw, none of which touches a device
//   test_jpeg_encode_images <block.bin> <preset> <subsampling> <out prefix> <w> <h> <colour type> <offset> [...]
//       the images described by the groups of four in the block -> <prefix>host<i>.jpg by encode_images (host form),
//       <prefix>device<i>.jpg by encode_images_device on an uploaded copy of the block and <prefix>loop<i>.jpg by a loop of
//       pixo::jpeg::encode over the same pixels; exits 1 when the three differ
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/pixo.hpp"

static pixo_png_image image(uint32_t w, uint32_t h, uint8_t ct, uint64_t at)
{
    pixo_png_image im{};
    im.width = w; im.height = h; im.color_type = ct; im.offset = at;
    return im;
}

template <class F> static bool throws(F &&call, pixo::Error::Kind kind, const char *what)
{
    try {
        (void)call();
    } catch (const pixo::Error &e) {
        if (e.kind() == kind && std::strstr(e.what(), what)) return true;
        std::printf("threw '%s', expected '%s'\n", e.what(), what);
        return false;
    }
    std::printf("did not throw: %s\n", what);
    return false;
}

static void write_file(const std::string &path, const std::vector<uint8_t> &f)
{
    std::ofstream(path, std::ios::binary).write(reinterpret_cast<const char *>(f.data()), (std::streamsize)f.size());
}

// The runtime's allocator and copy, looked up in the library the C ABI is linked against (this program includes no HIP header)
struct Device {
    int (*malloc_)(void **, size_t) = nullptr;
    int (*memcpy_)(void *, const void *, size_t, int) = nullptr;
    int (*free_)(void *) = nullptr;
    bool load()
    {
        void *h = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return false;
        malloc_ = reinterpret_cast<int (*)(void **, size_t)>(dlsym(h, "hipMalloc"));
        memcpy_ = reinterpret_cast<int (*)(void *, const void *, size_t, int)>(dlsym(h, "hipMemcpy"));
        free_ = reinterpret_cast<int (*)(void *)>(dlsym(h, "hipFree"));
        return malloc_ && memcpy_ && free_;
    }
};

int main(int argc, char **argv)
{
    using pixo::Error;
    namespace J = pixo::jpeg;
    if (argc == 2 && !std::strcmp(argv[1], "checks")) {
        const J::JpegOptions o = J::JpegOptions::fast(0, 0, 80); // (the template's own size is not read)
        const std::vector<uint8_t> block(80, 0);
        const std::vector<pixo_png_image> good{image(4, 4, 2, 0), image(5, 3, 0, 64)};
        bool ok = throws([&] { return J::encode_images(block.data(), 80, {}, o); }, Error::Kind::CompressionError, "batch must be 1..65535");
        ok = throws([&] { return J::encode_images(nullptr, 80, good, o); }, Error::Kind::CompressionError, "null argument 'data'") && ok;
        ok = throws([&] { return J::encode_images_device(nullptr, good, o); }, Error::Kind::CompressionError, "null argument 'd_pixels'") && ok;
        ok = throws([&] { return J::encode_images(block, good, J::JpegOptions::fast(0, 0, 0)); }, Error::Kind::InvalidQuality, "Invalid quality 0") && ok;
        ok = throws([&] { return J::encode_images(block.data(), 78, good, o); }, Error::Kind::InvalidDataLength, "expected 79 bytes, got 78") && ok;
        ok = throws([&] { return J::encode_images(block, {image(4, 4, 2, 0), image(0, 3, 0, 64)}, o); }, Error::Kind::InvalidDimensions,
                    "Invalid image dimensions: 0x3 (image 1)") && ok;
        ok = throws([&] { return J::encode_images(block, {image(4, 4, 3, 0)}, o); }, Error::Kind::UnsupportedColorType,
                    "Unsupported color type for this format (image 0)") && ok;
        ok = throws([&] { return J::encode_images_device(block.data(), {image(70000, 4, 2, 0)}, o); }, Error::Kind::ImageTooLarge,
                    "Image 70000x4 exceeds maximum dimension 65535 (image 0)") && ok;
        if (ok) std::puts("all checks passed");
        return ok ? 0 : 1;
    }
    if (argc < 9 || (argc - 5) % 4 != 0) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> block((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const uint8_t preset = (uint8_t)std::atoi(argv[2]);
    const J::Subsampling ss = std::atoi(argv[3]) ? J::Subsampling::S420 : J::Subsampling::S444;
    const std::string prefix = argv[4];
    std::vector<pixo_png_image> images;
    for (int a = 5; a < argc; a += 4)
        images.push_back(image((uint32_t)std::atoi(argv[a]), (uint32_t)std::atoi(argv[a + 1]), (uint8_t)std::atoi(argv[a + 2]), (uint64_t)std::atoll(argv[a + 3])));
    const J::JpegOptions o = J::JpegOptions::builder(0, 0).quality(80).preset(preset).subsampling(ss).build();
    const std::vector<std::vector<uint8_t>> host = J::encode_images(block, images, o);
    Device dev;
    void *d_block = nullptr;
    if (!dev.load() || dev.malloc_(&d_block, block.size()) != 0 || dev.memcpy_(d_block, block.data(), block.size(), /*hipMemcpyHostToDevice=*/1) != 0) {
        std::puts("no device memory for the block");
        return 1;
    }
    const std::vector<std::vector<uint8_t>> device = J::encode_images_device(d_block, images, o);
    (void)dev.free_(d_block);
    if (host.size() != images.size() || device.size() != images.size()) return 1;
    bool same = true;
    for (size_t i = 0; i < images.size(); ++i) {
        J::JpegOptions one = o;
        one.width = images[i].width; one.height = images[i].height;
        one.color_type = static_cast<pixo::ColorType>(images[i].color_type);
        const size_t bytes = (size_t)images[i].width * images[i].height * pixo::bytes_per_pixel(one.color_type);
        const std::vector<uint8_t> single = J::encode(block.data() + images[i].offset, bytes, one);
        if (single != host[i] || single != device[i]) { std::printf("file %zu differs from the loop's\n", i); same = false; }
        write_file(prefix + "host" + std::to_string(i) + ".jpg", host[i]);
        write_file(prefix + "device" + std::to_string(i) + ".jpg", device[i]);
        write_file(prefix + "loop" + std::to_string(i) + ".jpg", single);
    }
    if (same) std::puts("all checks passed");
    return same ? 0 : 1;
}
