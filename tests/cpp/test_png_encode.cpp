// TEST HARNESS — pixo::png::encode of include/pixo.hpp called once: test_png_encode <pixels.bin> <w> <h> <preset> <out.png>
// (RGBA pixels).  An invalid call must throw the error the C ABI reports.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../include/pixo.hpp"

int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> px((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]);
    pixo::png::PngOptions o = pixo::png::PngOptions::from_preset(w, h, (uint8_t)std::atoi(argv[4]));
    o.flags = PIXO_PNG_NO_RAYON;
    const std::vector<uint8_t> file = pixo::png::encode(px, o);
    std::ofstream(argv[5], std::ios::binary).write(reinterpret_cast<const char *>(file.data()), (std::streamsize)file.size());
    bool threw = false;
    try {
        (void)pixo::png::encode(px.data(), px.size() - 1, o);
    } catch (const pixo::Error &) {
        threw = true;
    }
    if (!threw) { std::puts("a short pixel buffer did not throw"); return 1; }
    std::puts("all checks passed");
    return 0;
}
