// png_reduce_math.h — per-pixel / per-group arithmetic of the PNG reductions (png_reduce.hip), written so that it also
// compiles for the host (tests/emu_png_reduce/): colour keys and their hash set, the byte of a reduced row, and the palette
// ordering that runs on the host in both builds.  Reference: src/png/mod.rs:633-1120, src/png/bit_depth.rs.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PNGR_HD __host__ __device__ __forceinline__
#else
#define PNGR_HD inline
#endif

namespace pixo_pngr {

// What a convert pass makes of the source pixels.  Every form is a pure function of (row, byte within the row).
enum Form : uint32_t {
    FORM_INDEX = 0,      // palette indices (src = the sorted-key index image, 1 byte per pixel) through `map`, packed at `bits`
    FORM_GRAY = 1,       // first channel of every pixel, packed at `bits` (RGB / RGBA -> Gray)
    FORM_RGB = 2,        // RGBA -> RGB
    FORM_GA = 3,         // RGBA -> GrayAlpha (r, a); with zero_alpha: gray 0 where a == 0
    FORM_ZERO_ALPHA = 4, // same pixel format (RGBA or GrayAlpha), colour channels 0 where alpha == 0
};

struct ConvertArgs {
    uint32_t form, spp, bits, zero_alpha; // spp: source bytes per pixel
    uint32_t width, height, row_bytes;    // row_bytes: bytes of one reduced row
};

// build_palette's key (mod.rs:855-872): r<<24 | g<<16 | b<<8 | a, RGB with a = 255
template <int SPP> PNGR_HD uint32_t color_key(const uint8_t *px)
{
    static_assert(SPP == 3 || SPP == 4, "palettes are built from RGB and RGBA only");
    return ((uint32_t)px[0] << 24) | ((uint32_t)px[1] << 16) | ((uint32_t)px[2] << 8) | (SPP == 4 ? (uint32_t)px[3] : 255u);
}

// Hash sets of colour keys: kSetSlots open-addressed 64-bit slots, a slot = kSlotUsed | value << 32 | key (value: 0 in the
// analysis, the sorted index in the lookup table).  At most 257 keys are ever inserted, so probing ends.
constexpr uint32_t kSetSlots = 1024;
constexpr uint64_t kSlotUsed = 1ull << 63;
PNGR_HD uint32_t key_hash(uint32_t k)
{
    k ^= k >> 15; k *= 0x2C1B3C6Du; k ^= k >> 12; k *= 0x297A2D39u; k ^= k >> 15;
    return k & (kSetSlots - 1);
}
PNGR_HD uint32_t lookup_index(const uint64_t *table, uint32_t key)
{
    for (uint32_t s = key_hash(key);; s = (s + 1) & (kSetSlots - 1)) {
        const uint64_t e = table[s];
        if ((uint32_t)e == key && (e & kSlotUsed)) return (uint32_t)(e >> 32) & 0xFFu;
        if (!(e & kSlotUsed)) return 0; // (not reached: every pixel's key is in the table)
    }
}

// One sample of a reduced row before packing: pixel x of row y
PNGR_HD uint32_t sample(const ConvertArgs &a, const uint8_t *src, const uint8_t *map, uint64_t pixel)
{
    return a.form == FORM_INDEX ? map[src[pixel]] : src[pixel * a.spp];
}

// Byte j of reduced row y.  Packing is MSB first, a row's last byte padded with zero bits (bit_depth.rs:105-148).
PNGR_HD uint8_t reduced_byte(const ConvertArgs &a, const uint8_t *src, const uint8_t *map, uint32_t y, uint32_t j)
{
    const uint64_t row0 = (uint64_t)y * a.width;
    switch (a.form) {
    case FORM_INDEX:
    case FORM_GRAY: {
        if (a.bits == 8) return (uint8_t)sample(a, src, map, row0 + j);
        const uint32_t per = 8 / a.bits, mask = (1u << a.bits) - 1;
        uint32_t acc = 0;
        for (uint32_t k = 0; k < per; ++k) {
            const uint32_t x = j * per + k;
            acc = (acc << a.bits) | (x < a.width ? (sample(a, src, map, row0 + x) & mask) : 0u);
        }
        return (uint8_t)acc;
    }
    case FORM_RGB: return src[(row0 + j / 3) * 4 + j % 3];
    case FORM_GA: {
        const uint8_t *p = src + (row0 + j / 2) * 4;
        if (j & 1) return p[3];
        return (a.zero_alpha && p[3] == 0) ? 0 : p[0];
    }
    default: { // FORM_ZERO_ALPHA (mod.rs:633-671)
        const uint32_t c = j % a.spp;
        const uint8_t *p = src + (row0 + j / a.spp) * a.spp;
        return (c + 1 < a.spp && p[a.spp - 1] == 0) ? 0 : p[c];
    }
    }
}

// palette_bit_depth / reduce_gray_bit_depth (bit_depth.rs:18-46)
inline uint32_t palette_bits(uint32_t n) { return n == 0 ? 8 : n <= 2 ? 1 : n <= 4 ? 2 : n <= 16 ? 4 : 8; }
inline uint32_t gray_bits(uint32_t max) { return max <= 1 ? 1 : max <= 3 ? 2 : max <= 15 ? 4 : 8; }

} // namespace pixo_pngr
