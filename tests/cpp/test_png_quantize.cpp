// TEST HARNESS: pixo::png::encode of include/pixo.hpp with quantisation — the options' own member and the explicit overload.
// usage: test_png_quantize <pixels.bin> <width> <height> <out_member.png> <out_overload.png> <out_off.png>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../include/pixo.hpp"

static void put(const char *path, const std::vector<uint8_t> &v)
{
    std::ofstream(path, std::ios::binary).write(reinterpret_cast<const char *>(v.data()), static_cast<std::streamsize>(v.size()));
}

int main(int argc, char **argv)
{
    if (argc != 7) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> px((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const uint32_t w = static_cast<uint32_t>(std::atoi(argv[2])), h = static_cast<uint32_t>(std::atoi(argv[3]));
    try {
        pixo::png::PngOptions lossy = pixo::png::PngOptions::from_preset_with_lossless(w, h, 1, false);
        lossy.color_type = pixo::ColorType::Rgb;
        lossy.flags = PIXO_PNG_NO_RAYON;
        if (lossy.quantization.mode != pixo::png::QuantizationMode::Auto || lossy.quantization.max_colors != 256 || !lossy.quantization.dithering) return 3;
        put(argv[4], pixo::png::encode(px, lossy)); // routes on the member
        pixo::png::PngOptions plain = pixo::png::PngOptions::from_preset_with_lossless(w, h, 1, true);
        plain.color_type = pixo::ColorType::Rgb;
        plain.flags = PIXO_PNG_NO_RAYON;
        if (plain.quantization.mode != pixo::png::QuantizationMode::Off) return 4;
        put(argv[5], pixo::png::encode(px.data(), px.size(), plain, lossy.quantization)); // the explicit overload
        put(argv[6], pixo::png::encode(px, plain));
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
