// png_quantize_math.h — the arithmetic of the PNG palette quantiser (png_quantize.hip), written so that it also compiles for
// the host (tests/emu_png_quantize/): colour keys, the Redmean distance, the first-minimum search, the 6-6-6 cell expansion and
// one Floyd-Steinberg step in its exact integer form.  Reference: src/png/mod.rs:1405-1499, :1634-1698.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PNGQ_HD __host__ __device__ __forceinline__
#else
#define PNGQ_HD inline
#endif

namespace pixo_pngq {

constexpr uint32_t kLutCells = 64 * 64 * 64; // (r6 << 12) | (g6 << 6) | b6
constexpr uint32_t kMaxPalette = 256;
constexpr uint32_t kBandRows = 64;           // rows of a dither band: one per lane of a wavefront

// quantize_image's key (mod.rs:1529-1535): r<<24 | g<<16 | b<<8 | a, RGB with a = 255.  A palette entry is kept in the same form.
PNGQ_HD uint32_t color_key(const uint8_t *px, uint32_t spp)
{
    return ((uint32_t)px[0] << 24) | ((uint32_t)px[1] << 16) | ((uint32_t)px[2] << 8) | (spp == 4 ? (uint32_t)px[3] : 255u);
}

// perceptual_distance_sq (mod.rs:1405-1430), all integer.  Never above 2^20: keys of (distance << 8 | index) fit 32 bits.
PNGQ_HD uint32_t distance(int32_t r1, int32_t g1, int32_t b1, int32_t a1, int32_t r2, int32_t g2, int32_t b2, int32_t a2)
{
    const int32_t dr = r1 - r2, dg = g1 - g2, db = b1 - b2, da = a1 - a2;
    const int32_t r_mean = (r1 + r2) >> 1;
    const int32_t d = ((512 + r_mean) * dr * dr + 1024 * dg * dg + (767 - r_mean) * db * db) >> 8;
    return (uint32_t)(d + da * da);
}
PNGQ_HD uint32_t distance_keys(uint32_t c, uint32_t p)
{
    return distance((int32_t)(c >> 24), (int32_t)((c >> 16) & 255), (int32_t)((c >> 8) & 255), (int32_t)(c & 255),
                    (int32_t)(p >> 24), (int32_t)((p >> 16) & 255), (int32_t)((p >> 8) & 255), (int32_t)(p & 255));
}

// nearest_palette_index (mod.rs:1432-1443): the FIRST entry at the minimum.  distance << 8 | index orders exactly so.
PNGQ_HD uint32_t nearest(const uint32_t *palette, uint32_t n, uint32_t color)
{
    uint32_t best = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = (distance_keys(color, palette[i]) << 8) | i;
        best = k < best ? k : best;
    }
    return best & 255u;
}

// PaletteLut (mod.rs:1457-1499): a cell's colour is its three 6-bit coordinates expanded to 8 bits, alpha 255
PNGQ_HD uint32_t expand6(uint32_t v) { return (v << 2) | (v >> 4); }
PNGQ_HD uint32_t cell_color(uint32_t cell) { return (expand6(cell >> 12) << 24) | (expand6((cell >> 6) & 63) << 16) | (expand6(cell & 63) << 8) | 255u; }
PNGQ_HD uint32_t cell_of(uint32_t r, uint32_t g, uint32_t b) { return ((r >> 2) << 12) | ((g >> 2) << 6) | (b >> 2); }
// lookup (:1487-1499): opaque colours through the table, every other alpha by the search
PNGQ_HD uint32_t lookup(const uint8_t *lut, const uint32_t *palette, uint32_t n, uint32_t r, uint32_t g, uint32_t b, uint32_t a)
{
    return a == 255 ? lut[cell_of(r, g, b)] : nearest(palette, n, (r << 24) | (g << 16) | (b << 8) | a);
}

// Floyd-Steinberg (mod.rs:1634-1698).  The reference's f32 accumulators only ever hold multiples of 1/16 below 2^12, so the
// loop is exact in integers: errors travel in sixteenths.  `in16` is what has been diffused into this pixel:
// 7 e[x-1] of its own row + (1 e[x-1] + 5 e[x] + 3 e[x+1]) of the row above.  (c + in16/16).clamp(0, 255) as u8:
PNGQ_HD int32_t dither_adjust(int32_t c, int32_t in16)
{
    const int32_t t = 16 * c + in16;
    return t < 0 ? 0 : ((t >> 4) > 255 ? 255 : (t >> 4));
}
// what a row hands to column x - 1 of the row below once it knows its errors at x - 2, x - 1 and x
PNGQ_HD int32_t dither_below(int32_t e_xm2, int32_t e_xm1, int32_t e_x) { return e_xm2 + 5 * e_xm1 + 3 * e_x; }

// Three such sums (each within +-9 * 255) and a "written" bit in one 64-bit word: what a band's last row leaves for the
// first row of the band below, column by column.
constexpr int32_t kCarryBias = 4096;
constexpr uint64_t kCarryValid = 1ull << 63;
PNGQ_HD uint64_t pack_carry(int32_t r, int32_t g, int32_t b)
{
    return kCarryValid | (uint64_t)(uint32_t)(r + kCarryBias) | ((uint64_t)(uint32_t)(g + kCarryBias) << 13) | ((uint64_t)(uint32_t)(b + kCarryBias) << 26);
}
PNGQ_HD void unpack_carry(uint64_t w, int32_t *r, int32_t *g, int32_t *b)
{
    *r = (int32_t)(w & 8191u) - kCarryBias;
    *g = (int32_t)((w >> 13) & 8191u) - kCarryBias;
    *b = (int32_t)((w >> 26) & 8191u) - kCarryBias;
}

// One pixel of the dither loop: colour c (r, g, b, a), incoming sixteenths -> index; errors out through e[3].
PNGQ_HD uint32_t dither_pixel(const uint8_t *lut, const uint32_t *palette, uint32_t n, const int32_t c[4], const int32_t in16[3], int32_t e[3])
{
    const int32_t r = dither_adjust(c[0], in16[0]), g = dither_adjust(c[1], in16[1]), b = dither_adjust(c[2], in16[2]);
    const uint32_t idx = lookup(lut, palette, n, (uint32_t)r, (uint32_t)g, (uint32_t)b, (uint32_t)c[3]);
    const uint32_t p = palette[idx];
    e[0] = r - (int32_t)(p >> 24);
    e[1] = g - (int32_t)((p >> 16) & 255);
    e[2] = b - (int32_t)((p >> 8) & 255);
    return idx;
}

} // namespace pixo_pngq
