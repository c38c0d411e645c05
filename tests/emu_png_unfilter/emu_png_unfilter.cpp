// TEST HARNESS — the per-byte arithmetic the PNG decoder's kernels run (pixo_amd/csrc/png_unfilter_math.h), compiled for the
// host and driven row by row and pixel by pixel: reconstruction of a whole stream, then the conversion to 8-bit pixels.
// emu_unfilter is also the single-thread loop tools/png_decode_timing.py times beside the reconstruction kernel.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../pixo_amd/csrc/png_unfilter_math.h"

using namespace pixo_pngu;

extern "C" uint32_t emu_pngu_paeth(uint32_t a, uint32_t b, uint32_t c) { return paeth(a, b, c); }
extern "C" uint32_t emu_pngu_reconstruct(uint32_t filter, uint32_t x, uint32_t a, uint32_t b, uint32_t c) { return reconstruct(filter, x, a, b, c); }
extern "C" uint32_t emu_pngu_filter_unit(uint32_t color_type, uint32_t depth) { return filter_unit(color_type, depth); }
extern "C" uint64_t emu_pngu_row_bytes(uint32_t color_type, uint32_t depth, uint32_t width) { return row_bytes(color_type, depth, width); }

// stream: height rows of 1 filter byte + rb bytes -> rows: height * rb bytes.  Returns the first row with a filter above 4, or -1.
extern "C" int64_t emu_pngu_unfilter(const uint8_t *stream, uint32_t height, uint64_t rb, uint32_t bpp, uint8_t *rows)
{
    std::vector<uint8_t> zero(rb, 0);
    for (uint32_t y = 0; y < height; ++y) {
        const uint8_t *src = stream + (uint64_t)y * (rb + 1);
        if (src[0] > FILTER_PAETH) return y;
        uint8_t *row = rows + (uint64_t)y * rb;
        std::memcpy(row, src + 1, rb);
        unfilter_row(src[0], row, y ? row - rb : zero.data(), rb, bpp);
    }
    return -1;
}

// rows (rb bytes apart) -> pixels; returns the bytes per output pixel
extern "C" uint32_t emu_pngu_convert(const uint8_t *rows, uint32_t width, uint32_t height, uint32_t color_type, uint32_t depth, const uint8_t *plte,
                                     uint32_t entries, const uint8_t *trns, uint32_t trns_len, uint8_t *out)
{
    const uint64_t rb = row_bytes(color_type, depth, width);
    const uint32_t form = convert_of(color_type, depth);
    const bool rgba = color_type == CT_INDEXED && trns_has_alpha(trns, trns_len);
    const uint32_t out_bpp = color_type == CT_INDEXED ? (rgba ? 4u : 3u) : channels(color_type);
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = color_type == CT_INDEXED ? palette_rgba(plte, entries, trns, rgba ? trns_len : 0, i) : 0;
    for (uint32_t y = 0; y < height; ++y) {
        const uint8_t *row = rows + y * rb;
        uint8_t *o = out + (uint64_t)y * width * out_bpp;
        if (form == CONVERT_COPY || form == CONVERT_HIGH)
            for (uint64_t i = 0; i < (uint64_t)width * out_bpp; ++i) o[i] = (uint8_t)convert_byte(form, row, i);
        else
            for (uint32_t x = 0; x < width; ++x) {
                const uint32_t v = convert_sample(form, row, x, depth, table);
                for (uint32_t k = 0; k < out_bpp; ++k) o[(uint64_t)x * out_bpp + k] = (uint8_t)(v >> (8 * k));
            }
    }
    return out_bpp;
}
