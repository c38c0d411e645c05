// TEST HARNESS — not product code.  Runs the arithmetic of the PNG quantisation kernels (pixo_amd/csrc/png_quantize_math.h:
// distance, first-minimum search, cell expansion, one dither step, the carry word between bands) on the host, in the
// kernels' order of work: the table is nearest(cell_color) per cell; a dithered image is dither_pixel per pixel with the
// sums dither_below hands from row to row, every sum passing through pack_carry / unpack_carry at a band boundary.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../pixo_amd/csrc/png_quantize_math.h"

using namespace pixo_pngq;

extern "C" {

uint32_t emu_pngq_distance(uint32_t c, uint32_t p) { return distance_keys(c, p); }
uint32_t emu_pngq_cell_color(uint32_t cell) { return cell_color(cell); }
uint32_t emu_pngq_nearest(const uint32_t *palette, uint32_t n, uint32_t color) { return nearest(palette, n, color); }
int32_t emu_pngq_dither_adjust(int32_t c, int32_t in16) { return dither_adjust(c, in16); }

void emu_pngq_lut(const uint32_t *palette, uint32_t n, uint8_t *lut)
{
    for (uint32_t cell = 0; cell < kLutCells; ++cell) lut[cell] = (uint8_t)nearest(palette, n, cell_color(cell));
}

// one pixel: colour key, incoming sixteenths -> index, errors
uint32_t emu_pngq_dither_pixel(const uint8_t *lut, const uint32_t *palette, uint32_t n, uint32_t key, const int32_t *in16, int32_t *e)
{
    const int32_t c[4] = {(int32_t)(key >> 24), (int32_t)((key >> 16) & 255), (int32_t)((key >> 8) & 255), (int32_t)(key & 255)};
    return dither_pixel(lut, palette, n, c, in16, e);
}

// a whole image, row by row; rows that start a band take the sums of the row above through the carry word
void emu_pngq_dither_image(const uint32_t *keys, uint32_t w, uint32_t h, const uint8_t *lut, const uint32_t *palette, uint32_t n, uint8_t *index)
{
    std::vector<int32_t> above(3 * (size_t)w, 0), err(3 * ((size_t)w + 2), 0);
    for (uint32_t y = 0; y < h; ++y) {
        int32_t prev[3] = {0, 0, 0};
        std::vector<int32_t> mine(3 * ((size_t)w + 2), 0); // errors of this row at [x + 1]
        for (uint32_t x = 0; x < w; ++x) {
            const uint32_t key = keys[(size_t)y * w + x];
            const int32_t c[4] = {(int32_t)(key >> 24), (int32_t)((key >> 16) & 255), (int32_t)((key >> 8) & 255), (int32_t)(key & 255)};
            const int32_t in16[3] = {above[3 * x] + 7 * prev[0], above[3 * x + 1] + 7 * prev[1], above[3 * x + 2] + 7 * prev[2]};
            index[(size_t)y * w + x] = (uint8_t)dither_pixel(lut, palette, n, c, in16, prev);
            for (int k = 0; k < 3; ++k) mine[3 * (x + 1) + k] = prev[k];
        }
        for (uint32_t x = 0; x < w; ++x) { // column x of the row below: e[x - 1], e[x], e[x + 1]
            int32_t s[3];
            for (int k = 0; k < 3; ++k) s[k] = dither_below(mine[3 * x + k], mine[3 * (x + 1) + k], mine[3 * (x + 2) + k]);
            if ((y + 1) % kBandRows == 0) unpack_carry(pack_carry(s[0], s[1], s[2]), &s[0], &s[1], &s[2]);
            for (int k = 0; k < 3; ++k) above[3 * x + k] = s[k];
        }
    }
}
}
