// TEST HARNESS: the ragged resize form's host-and-device header (pixo_amd/csrc/resize_images_math.h) compiled for the host —
// the tile -> (image, tile x, tile y) search the kernels run, the tiles of an image per pass, the table of a sub-batch as the
// driver builds it, and a walk of a launch that marks what every workgroup's threads would write: the three bodies' index
// arithmetic (resize.hip) restated over counters instead of pixels.
#include "../../pixo_amd/csrc/resize_images_math.h"

using namespace pixo_resize_images;

struct LaunchC { uint32_t bpp, first_record, count, tiles; };

extern "C" {
uint32_t emu_record_bytes(void) { return (uint32_t)sizeof(Record); }
uint32_t emu_item_bytes(void) { return (uint32_t)sizeof(Item); }
uint32_t emu_image_of_tile(const Record *t, uint32_t count, uint32_t tile) { return image_of_tile(t, count, tile); }
void emu_tile_in_image(uint32_t tile, uint32_t first_tile, uint32_t tiles_x, uint32_t *tx, uint32_t *ty) { tile_in_image(tile, first_tile, tiles_x, tx, ty); }
void emu_tiles_of(int pass, uint32_t sh, uint32_t dw, uint32_t dh, uint32_t bpp, uint32_t rows_cap, uint32_t *tx, uint32_t *ty)
{
    tiles_of(pass, sh, dw, dh, bpp, rows_cap, tx, ty);
}
uint64_t emu_tile_count(int pass, uint32_t sh, uint32_t dw, uint32_t dh, uint32_t bpp, uint32_t rows_cap) { return tile_count(pass, sh, dw, dh, bpp, rows_cap); }
// -> the number of launches, or -1 when build_table refuses; `table`, `launches` and `record_item` have room for n entries
int emu_build_table(const Item *items, uint32_t n, int pass, uint32_t rows_cap, Record *table, LaunchC *launches, uint32_t *record_item)
{
    std::vector<Item> in(items, items + n);
    std::vector<Record> t;
    std::vector<Launch> l;
    std::vector<uint32_t> r;
    if (!build_table(in, pass, rows_cap, t, l, r)) return -1;
    for (size_t i = 0; i < t.size(); ++i) { table[i] = t[i]; record_item[i] = r[i]; }
    for (size_t i = 0; i < l.size(); ++i) launches[i] = LaunchC{l[i].bpp, l[i].first_record, l[i].count, l[i].tiles};
    return (int)l.size();
}
// Every workgroup of a launch of `tiles` tiles over `count` records, every thread of it: hits[record.dst + element] += 1 for
// every element the thread would store, with the bodies' loops.  An element is a destination pixel (PASS_POINT), a pixel of
// the intermediate indexed row * dw + column (PASS_H), a destination byte (PASS_V); record.dst is used as the image's first
// index into `hits`.  -> 0, or -1 when an index leaves [0, n_hits).
int emu_cover(const Record *t, uint32_t count, uint32_t tiles, int pass, uint32_t *hits, uint64_t n_hits)
{
    for (uint32_t tile = 0; tile < tiles; ++tile) {
        const Record &im = t[image_of_tile(t, count, tile)];
        uint32_t tx, ty;
        tile_in_image(tile, im.first_tile, im.tiles_x, &tx, &ty);
        if (tx >= im.tiles_x || ty >= im.tiles_y) return -1;
        if (pass == PASS_POINT) {
            for (uint32_t lane_y = 0; lane_y < 4; ++lane_y)
                for (uint32_t lane_x = 0; lane_x < 64; ++lane_x) {
                    const uint64_t gx = (uint64_t)tx * 64 + lane_x;
                    if (gx * 4 >= im.dw) continue;
                    const uint32_t x_first = (uint32_t)(gx * 4), pixels = im.dw - x_first < 4 ? im.dw - x_first : 4;
                    for (uint64_t y = (uint64_t)ty * 4 + lane_y; y < im.dh; y += (uint64_t)im.tiles_y * 4)
                        for (uint32_t k = 0; k < pixels; ++k) {
                            const uint64_t at = im.dst + y * im.dw + x_first + k;
                            if (at >= n_hits) return -1;
                            hits[at] += 1;
                        }
                }
        } else if (pass == PASS_H) {
            for (uint64_t yb = (uint64_t)ty * 4; yb < im.sh; yb += (uint64_t)im.tiles_y * 4)
                for (uint32_t lane_y = 0; lane_y < 4; ++lane_y)
                    for (uint32_t lane_x = 0; lane_x < 64; ++lane_x) {
                        const uint64_t d = (uint64_t)tx * 64 + lane_x, y = yb + lane_y;
                        if (!(y < im.sh && d < im.dw)) continue;
                        const uint64_t at = im.dst + y * im.dw + d;
                        if (at >= n_hits) return -1;
                        hits[at] += 1;
                    }
        } else {
            const uint64_t row_bytes = (uint64_t)im.dw * im.bpp;
            for (uint32_t lane = 0; lane < 256; ++lane) {
                const uint64_t b = ((uint64_t)tx * 256 + lane) * 4;
                if (b >= row_bytes) continue;
                const uint32_t n = row_bytes - b < 4 ? (uint32_t)(row_bytes - b) : 4;
                for (uint64_t y = ty; y < im.dh; y += im.tiles_y)
                    for (uint32_t k = 0; k < n; ++k) {
                        const uint64_t at = im.dst + y * row_bytes + b + k;
                        if (at >= n_hits) return -1;
                        hits[at] += 1;
                    }
            }
        }
    }
    return 0;
}
}
