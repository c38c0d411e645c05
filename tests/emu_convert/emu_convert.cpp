// TEST HARNESS: the colour conversion's host-and-device header (pixo_amd/csrc/convert_math.h) compiled for the host — the
// kinds, the luma, the 16-pixel step, the tile -> image search the kernels run, the tiles of an image, the table of a
// sub-batch as the driver builds it, the whole lane body over host memory (every workgroup, every lane of a launch), and a
// walk that counts how often every output byte is written (the body's index arithmetic restated over counters).
#include "../../pixo_amd/csrc/convert_math.h"

using namespace pixo_convert;

struct LaunchC { uint32_t cls, first_record, count, tiles; };

// lane_body<kind, form> chosen at run time, as the launchers of convert.hip choose the kernel
static void run_lane(int kind, int form, const uint8_t *src, uint8_t *dst, uint64_t pixels, uint32_t bpp, uint32_t tile, uint32_t tiles, uint32_t lane)
{
#define EMU_CV(K)                                                                            \
    case K:                                                                                  \
        if (form == F_ALIGNED) lane_body<K, F_ALIGNED>(src, dst, pixels, bpp, tile, tiles, lane); \
        else lane_body<K, F_BYTES>(src, dst, pixels, bpp, tile, tiles, lane);                \
        break
    switch (kind) { EMU_CV(K_COPY); EMU_CV(K_GA_G); EMU_CV(K_RGBA_RGB); EMU_CV(K_RGB_G); EMU_CV(K_RGBA_G); }
#undef EMU_CV
}
// Every workgroup of a launch of `tiles` tiles over `count` records of class (kind, form), every lane of it, over the host
// memory the records point at.  -> 0, or -1 when a tile lands outside its image's tiles.
static int run_launch(const Record *t, uint32_t count, uint32_t tiles, int kind, int form)
{
    for (uint32_t tile = 0; tile < tiles; ++tile) {
        const Record &im = t[image_of_tile(t, count, tile)];
        if (tile < im.first_tile || tile - im.first_tile >= im.tiles) return -1;
        for (uint32_t lane = 0; lane < kWorkgroup; ++lane)
            run_lane(kind, form, reinterpret_cast<const uint8_t *>(im.src), reinterpret_cast<uint8_t *>(im.dst), im.pixels, im.bpp,
                     tile - im.first_tile, im.tiles, lane);
    }
    return 0;
}

extern "C" {
uint32_t emu_cv_record_bytes(void) { return (uint32_t)sizeof(Record); }
uint32_t emu_cv_item_bytes(void) { return (uint32_t)sizeof(Item); }
uint32_t emu_cv_tile_pixels(void) { return kTilePixels; }
uint32_t emu_cv_image_tiles(void) { return kImageTiles; }
int emu_cv_kind_of(uint32_t src_ct, uint32_t dst_ct) { return kind_of(src_ct, dst_ct); }
int emu_cv_target_type(uint32_t target, uint32_t src_ct) { return target_type(target, src_ct); }
uint32_t emu_cv_image_of_tile(const Record *t, uint32_t count, uint32_t tile) { return image_of_tile(t, count, tile); }
uint32_t emu_cv_tiles_of(uint64_t pixels, uint32_t image_tiles) { return tiles_of(pixels, image_tiles); }
// -> the number of launches, or -1 when build_table refuses; `table`, `launches` and `record_item` have room for n entries
int emu_cv_build_table(const Item *items, uint32_t n, uint32_t image_tiles, uint64_t launch_tiles, Record *table, LaunchC *launches, uint32_t *record_item)
{
    std::vector<Item> in(items, items + n);
    std::vector<Record> t;
    std::vector<Launch> l;
    std::vector<uint32_t> r;
    if (!build_table(in, image_tiles, launch_tiles, t, l, r)) return -1;
    for (size_t i = 0; i < t.size(); ++i) { table[i] = t[i]; record_item[i] = r[i]; }
    for (size_t i = 0; i < l.size(); ++i) launches[i] = LaunchC{l[i].cls, l[i].first_record, l[i].count, l[i].tiles};
    return (int)l.size();
}
// out[(r << 16) | (g << 8) | b] = luma(r, g, b), all 2^24 of them
void emu_cv_luma_all(uint8_t *out)
{
    for (uint32_t i = 0; i < (1u << 24); ++i) out[i] = (uint8_t)luma(i >> 16, (i >> 8) & 255u, i & 255u);
}
// The 16-pixel step of `kind` (1..4) over `groups` groups: 16 * source-bpp bytes each in, 16 * destination-bpp each out
void emu_cv_convert16(int kind, const uint8_t *in, uint8_t *out, uint32_t groups)
{
    const uint32_t sb = src_bpp(kind, 0), db = dst_bpp(kind, 0);
    for (uint32_t g = 0; g < groups; ++g) {
        uint32_t wi[16] = {0}, wo[12] = {0};
        for (uint32_t i = 0; i < 16 * sb; ++i) wi[i >> 2] |= (uint32_t)in[g * 16 * sb + i] << (8 * (i & 3));
        if (kind == K_GA_G) convert16<K_GA_G>(wi, wo);
        else if (kind == K_RGBA_RGB) convert16<K_RGBA_RGB>(wi, wo);
        else if (kind == K_RGB_G) convert16<K_RGB_G>(wi, wo);
        else convert16<K_RGBA_G>(wi, wo);
        for (uint32_t i = 0; i < 16 * db; ++i) out[g * 16 * db + i] = (uint8_t)(wo[i >> 2] >> (8 * (i & 3)));
    }
}
int emu_cv_run_launch(const Record *t, uint32_t count, uint32_t tiles, int kind, int form) { return run_launch(t, count, tiles, kind, form); }
// hits[record.dst + byte] += 1 for every destination byte a lane of the launch would store, with lane_body's loop of 16 pixels a lane
// (the four conversions' aligned form and every byte form; the aligned copy deals the same tile's bytes out quad by quad); record.dst is
// used as the image's first index into `hits`, dbpp: destination bytes per pixel.  -> 0, or -1 when an index leaves [0, n_hits).
int emu_cv_cover(const Record *t, uint32_t count, uint32_t tiles, uint32_t dbpp, uint32_t *hits, uint64_t n_hits)
{
    for (uint32_t tile = 0; tile < tiles; ++tile) {
        const Record &im = t[image_of_tile(t, count, tile)];
        if (tile < im.first_tile || tile - im.first_tile >= im.tiles) return -1;
        for (uint32_t lane = 0; lane < kWorkgroup; ++lane)
            for (uint64_t tt = tile - im.first_tile; tt * kTilePixels < im.pixels; tt += im.tiles) {
                const uint64_t first = tt * kTilePixels + (uint64_t)lane * kLanePixels;
                if (first >= im.pixels) break;
                const uint64_t n = im.pixels - first < kLanePixels ? im.pixels - first : kLanePixels;
                for (uint64_t b = first * dbpp; b < (first + n) * dbpp; ++b) {
                    if (im.dst + b >= n_hits) return -1;
                    hits[im.dst + b] += 1;
                }
            }
    }
    return 0;
}
}
