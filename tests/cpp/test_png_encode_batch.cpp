// TEST HARNESS — pixo::png::encode_batch of include/pixo.hpp.
//   test_png_encode_batch checks                                   the calls that must throw, none of which touches a device
//   test_png_encode_batch <pixels.bin> <w> <h> <preset> <batch> <out prefix>   RGBA pixels of `batch` images -> <prefix><i>.png
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/pixo.hpp"

static bool throws(const uint8_t *px, size_t len, const pixo::png::PngOptions &o, uint32_t batch, const char *what)
{
    try {
        (void)pixo::png::encode_batch(px, len, o, batch);
    } catch (const pixo::Error &e) {
        if (std::strstr(e.what(), what)) return true;
        std::printf("threw '%s', expected '%s'\n", e.what(), what);
        return false;
    }
    std::printf("did not throw: %s\n", what);
    return false;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "checks")) {
        const pixo::png::PngOptions o = pixo::png::PngOptions::fast(4, 4);
        const std::vector<uint8_t> two(2 * 64, 0);
        bool ok = throws(two.data(), 128, o, 0, "expected 0 bytes, got 128"); // batch x one image is the expected length
        ok = throws(two.data(), 0, o, 0, "batch must be 1..65535") && ok;
        ok = throws(nullptr, 128, o, 2, "null argument 'pixels'") && ok;
        ok = throws(two.data(), 128, o, 3, "expected 192 bytes, got 128") && ok;
        ok = throws(two.data(), 64, o, 2, "expected 128 bytes, got 64") && ok;
        if (ok) std::puts("all checks passed");
        return ok ? 0 : 1;
    }
    if (argc != 7) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> px((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]), batch = (uint32_t)std::atoi(argv[5]);
    const pixo::png::PngOptions o = pixo::png::PngOptions::from_preset(w, h, (uint8_t)std::atoi(argv[4]));
    const std::vector<std::vector<uint8_t>> files = pixo::png::encode_batch(px, o, batch);
    if (files.size() != batch) return 1;
    for (uint32_t i = 0; i < batch; ++i)
        std::ofstream(std::string(argv[6]) + std::to_string(i) + ".png", std::ios::binary).write(reinterpret_cast<const char *>(files[i].data()), (std::streamsize)files[i].size());
    std::puts("all checks passed");
    return 0;
}
