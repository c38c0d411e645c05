// TEST HARNESS — not product code.  Runs the per-byte arithmetic of the PNG reduction kernels
// (pixo_amd/csrc/png_reduce_math.h: colour keys, the key lookup table, reduced_byte) on the host, in the kernels' order
// of work: a convert pass is reduced_byte for every (row, byte); an index pass is color_key + lookup_index per pixel.
#include <cstdint>
#include <cstring>

#include "../../pixo_amd/csrc/png_reduce_math.h"

using namespace pixo_pngr;

extern "C" {

// form / spp / bits / zero_alpha as ConvertArgs; out: height * row_bytes bytes
int emu_png_convert(const uint8_t *src, const uint8_t *map, uint32_t form, uint32_t spp, uint32_t bits, uint32_t zero_alpha,
                    uint32_t width, uint32_t height, uint32_t row_bytes, uint8_t *out)
{
    ConvertArgs a{form, spp, bits, zero_alpha, width, height, row_bytes};
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t j = 0; j < row_bytes; ++j) out[(uint64_t)y * row_bytes + j] = reduced_byte(a, src, map, y, j);
    return 0;
}

// sorted keys -> lookup table (as the host builds it), then every pixel's index through it.  spp 3 or 4.
int emu_png_index(const uint8_t *px, uint64_t pixels, uint32_t spp, const uint32_t *sorted_keys, uint32_t n, uint8_t *index)
{
    static uint64_t table[kSetSlots];
    std::memset(table, 0, sizeof(table));
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t s = key_hash(sorted_keys[i]);
        while (table[s] & kSlotUsed) s = (s + 1) & (kSetSlots - 1);
        table[s] = kSlotUsed | ((uint64_t)i << 32) | sorted_keys[i];
    }
    for (uint64_t p = 0; p < pixels; ++p)
        index[p] = (uint8_t)lookup_index(table, spp == 4 ? color_key<4>(px + 4 * p) : color_key<3>(px + 3 * p));
    return 0;
}

uint32_t emu_png_palette_bits(uint32_t n) { return palette_bits(n); }
uint32_t emu_png_gray_bits(uint32_t max) { return gray_bits(max); }
}
