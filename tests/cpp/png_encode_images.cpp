// TEST HARNESS — pixo::png::encode_images of include/pixo.hpp.
//   png_encode_images checks                          the calls that must throw, none of which touches a device
//   png_encode_images <block.bin> <preset> <out prefix> <w> <h> <colour type> <offset> [...]
//       the images described by the groups of four in the block -> <prefix>images<i>.png by encode_images and
//       <prefix>loop<i>.png by a loop of pixo::png::encode over the same pixels; exits 1 when the two differ
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

static bool throws(const uint8_t *block, size_t len, const std::vector<pixo_png_image> &images, const pixo::png::PngOptions &o, const char *what)
{
    try {
        (void)pixo::png::encode_images(block, len, images, o);
    } catch (const pixo::Error &e) {
        if (std::strstr(e.what(), what)) return true;
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

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "checks")) {
        const pixo::png::PngOptions o = pixo::png::PngOptions::fast(0, 0); // (the template's own size is not read)
        const std::vector<uint8_t> block(80, 0);
        const std::vector<pixo_png_image> good{image(4, 4, 3, 0), image(5, 3, 0, 64)};
        bool ok = throws(block.data(), 80, {}, o, "batch must be 1..65535");
        ok = throws(nullptr, 80, good, o, "null argument 'pixels'") && ok;
        ok = throws(block.data(), 78, good, o, "expected 79 bytes, got 78") && ok;
        ok = throws(block.data(), 80, {image(4, 4, 3, 0), image(0, 3, 0, 64)}, o, "Invalid image dimensions: 0x3 (image 1)") && ok;
        ok = throws(block.data(), 80, {image(4, 4, 7, 0)}, o, "Unsupported color type for this format (image 0)") && ok;
        if (ok) std::puts("all checks passed");
        return ok ? 0 : 1;
    }
    if (argc < 8 || (argc - 4) % 4 != 0) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> block((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const uint8_t preset = (uint8_t)std::atoi(argv[2]);
    const std::string prefix = argv[3];
    std::vector<pixo_png_image> images;
    for (int a = 4; a < argc; a += 4)
        images.push_back(image((uint32_t)std::atoi(argv[a]), (uint32_t)std::atoi(argv[a + 1]), (uint8_t)std::atoi(argv[a + 2]), (uint64_t)std::atoll(argv[a + 3])));
    const pixo::png::PngOptions o = pixo::png::PngOptions::from_preset(0, 0, preset);
    const std::vector<std::vector<uint8_t>> files = pixo::png::encode_images(block.data(), block.size(), images, o);
    if (files.size() != images.size()) return 1;
    bool same = true;
    for (size_t i = 0; i < images.size(); ++i) {
        pixo::png::PngOptions one = pixo::png::PngOptions::from_preset(images[i].width, images[i].height, preset);
        one.color_type = static_cast<pixo::ColorType>(images[i].color_type);
        const size_t bytes = (size_t)images[i].width * images[i].height * pixo::bytes_per_pixel(one.color_type);
        const std::vector<uint8_t> single = pixo::png::encode(block.data() + images[i].offset, bytes, one);
        if (single != files[i]) { std::printf("file %zu differs from the loop's\n", i); same = false; }
        write_file(prefix + "images" + std::to_string(i) + ".png", files[i]);
        write_file(prefix + "loop" + std::to_string(i) + ".png", single);
    }
    if (same) std::puts("all checks passed");
    return same ? 0 : 1;
}
