// png_unfilter_math.h — per-byte arithmetic of the PNG decoder's device stage (png_unfilter.hip), written so that it also
// compiles for the host (tests/emu_png_unfilter/, tools/png_decode_timing.py's baseline): the five row reconstructions, the
// geometry of a row, the unpacking of packed samples, their scaling to 8 bits and the palette lookup.
// Reference: src/decode/png.rs:294-626 (reconstruct_image, unfilter_row, paeth_predictor, convert_to_pixels, unpack_row,
// scale_to_8bit).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PNGU_HD __host__ __device__ __forceinline__
#else
#define PNGU_HD inline
#endif

namespace pixo_pngu {

// The colour type byte of IHDR (png.rs:31-38)
enum : uint32_t { CT_GRAY = 0, CT_RGB = 2, CT_INDEXED = 3, CT_GRAY_ALPHA = 4, CT_RGBA = 6 };
enum : uint32_t { FILTER_NONE = 0, FILTER_SUB = 1, FILTER_UP = 2, FILTER_AVERAGE = 3, FILTER_PAETH = 4 };

PNGU_HD uint32_t channels(uint32_t color_type)
{
    return color_type == CT_RGB ? 3u : color_type == CT_GRAY_ALPHA ? 2u : color_type == CT_RGBA ? 4u : 1u;
}
PNGU_HD bool depth_valid(uint32_t color_type, uint32_t depth) // png.rs:243-249
{
    if (color_type == CT_GRAY) return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
    if (color_type == CT_INDEXED) return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    return depth == 8 || depth == 16;
}
// The filter unit (png.rs:305-332): 1 for every palette depth and gray of 8 bits or fewer, 2 for 16-bit gray,
// channels * depth / 8 otherwise.
PNGU_HD uint32_t filter_unit(uint32_t color_type, uint32_t depth)
{
    if (color_type == CT_INDEXED) return 1;
    if (color_type == CT_GRAY) return depth == 16 ? 2u : 1u;
    return channels(color_type) * depth / 8;
}
// Bytes of a row without its filter byte (png.rs:84-90)
PNGU_HD uint64_t row_bytes(uint32_t color_type, uint32_t depth, uint32_t width)
{
    if (color_type == CT_GRAY || color_type == CT_INDEXED) return ((uint64_t)width * depth + 7) / 8;
    return (uint64_t)width * channels(color_type) * depth / 8;
}

// paeth_predictor (png.rs:414-427): ties resolve as a, then b, then c
PNGU_HD uint32_t paeth(uint32_t a, uint32_t b, uint32_t c)
{
    const int p = (int)a + (int)b - (int)c;
    int pa = p - (int)a, pb = p - (int)b, pc = p - (int)c;
    pa = pa < 0 ? -pa : pa;
    pb = pb < 0 ? -pb : pb;
    pc = pc < 0 ? -pc : pc;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// One reconstructed byte (unfilter_row, png.rs:370-410): x the filtered byte, a left, b above, c above-left (0 where the
// reference has none).  Sums wrap modulo 256; Average is the floor of the 9-bit sum.  `filter` is 0..4.
PNGU_HD uint32_t reconstruct(uint32_t filter, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t pred = filter == FILTER_SUB ? a : filter == FILTER_UP ? b : filter == FILTER_AVERAGE ? (a + b) >> 1
                        : filter == FILTER_PAETH ? paeth(a, b, c) : 0u;
    return (x + pred) & 255u;
}
// A whole row in place, as the reference walks it: `prev` is the reconstructed row above (zeros above row 0).
PNGU_HD void unfilter_row(uint32_t filter, uint8_t *row, const uint8_t *prev, size_t n, uint32_t bpp)
{
    for (size_t i = 0; i < n; ++i) {
        const uint32_t a = i >= bpp ? row[i - bpp] : 0u, c = i >= bpp ? prev[i - bpp] : 0u;
        row[i] = (uint8_t)reconstruct(filter, row[i], a, prev[i], c);
    }
}

// unpack_row (png.rs:567-609): sample x of a row packed MSB first at `depth` bits (1, 2, 4 or 8)
PNGU_HD uint32_t unpack_sample(const uint8_t *row, uint64_t x, uint32_t depth)
{
    if (depth == 8) return row[x];
    const uint32_t per = 8 / depth;
    const uint32_t shift = (per - 1 - (uint32_t)(x % per)) * depth;
    return (row[x / per] >> shift) & ((1u << depth) - 1);
}
// scale_to_8bit (png.rs:612-626): 1 bit to 0 / 255, 2 and 4 bits by bit replication
PNGU_HD uint32_t scale_to_8bit(uint32_t s, uint32_t depth)
{
    if (depth == 1) return s ? 255u : 0u;
    if (depth == 2) return (s | (s << 2) | (s << 4) | (s << 6)) & 255u;
    if (depth == 4) return (s | (s << 4)) & 255u;
    return s;
}
// Palette entry `idx` as r | g << 8 | b << 16 | a << 24 (png.rs:501-517): an index beyond the palette is opaque black,
// alpha beyond tRNS is 255.
PNGU_HD uint32_t palette_rgba(const uint8_t *plte, uint32_t entries, const uint8_t *trns, uint32_t trns_len, uint32_t idx)
{
    if (idx >= entries) return 0xFF000000u;
    const uint32_t a = idx < trns_len ? trns[idx] : 255u;
    return (uint32_t)plte[3 * idx] | ((uint32_t)plte[3 * idx + 1] << 8) | ((uint32_t)plte[3 * idx + 2] << 16) | (a << 24);
}
// has_alpha_in_trns (png.rs:70-72)
PNGU_HD bool trns_has_alpha(const uint8_t *trns, uint32_t trns_len)
{
    for (uint32_t i = 0; i < trns_len; ++i)
        if (trns[i] != 255) return true;
    return false;
}

// What the conversion pass makes of the reconstructed rows (convert_to_pixels, png.rs:430-533).
enum Convert : uint32_t {
    CONVERT_COPY = 0,    // 8-bit gray, gray+alpha, RGB, RGBA: the row bytes
    CONVERT_HIGH = 1,    // 16-bit samples: the high byte of each
    CONVERT_GRAY = 2,    // gray at 1, 2, 4 bits: unpacked and scaled
    CONVERT_PALETTE = 3, // palette indices at 1, 2, 4, 8 bits through the table, 3 or 4 bytes a pixel
};
PNGU_HD uint32_t convert_of(uint32_t color_type, uint32_t depth)
{
    if (color_type == CT_INDEXED) return CONVERT_PALETTE;
    if (depth == 16) return CONVERT_HIGH;
    return depth == 8 ? CONVERT_COPY : CONVERT_GRAY;
}
// Output byte i of a row for the two byte-wise forms
PNGU_HD uint32_t convert_byte(uint32_t form, const uint8_t *row, uint64_t i) { return form == CONVERT_HIGH ? row[2 * i] : row[i]; }
// Output pixel x of a row for the two sample-wise forms: gray -> the byte; palette -> the table's word
PNGU_HD uint32_t convert_sample(uint32_t form, const uint8_t *row, uint64_t x, uint32_t depth, const uint32_t *table)
{
    const uint32_t s = unpack_sample(row, x, depth);
    return form == CONVERT_GRAY ? scale_to_8bit(s, depth) : table[s];
}

} // namespace pixo_pngu
