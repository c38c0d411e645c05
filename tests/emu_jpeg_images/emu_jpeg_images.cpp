// TEST HARNESS: pixo_amd/csrc/jpeg_images_math.h compiled for the host, behind a C interface for tests/test_emu_jpeg_images.py.
// The searches are the templates the kernels instantiate (there over a pointer into the constant address space).
#include <cstring>

#include "../../pixo_amd/csrc/jpeg_images_math.h"

namespace ji = pixo_jpeg_images;

extern "C" {

uint32_t emu_ji_tile_record_bytes() { return sizeof(ji::TileRecord); }
uint32_t emu_ji_seg_record_bytes() { return sizeof(ji::SegRecord); }
uint32_t emu_ji_image_of_tile(const ji::TileRecord *t, uint32_t count, uint32_t tile) { return ji::image_of_tile(t, count, tile); }
uint32_t emu_ji_segment_of_group(const ji::SegRecord *t, uint32_t count, uint32_t group) { return ji::segment_of_group(t, count, group); }
void emu_ji_shape_of(int mode, uint32_t w, uint32_t h, uint32_t out[6])
{
    const ji::Shape s = ji::shape_of(mode, w, h);
    out[0] = s.units_x; out[1] = s.units_y; out[2] = s.tiles_x; out[3] = s.tiles_y; out[4] = s.y_blocks; out[5] = s.c_blocks;
}
int emu_ji_load_form_of(uint64_t address, uint32_t w, uint32_t bpp) { return ji::load_form_of(address, w, bpp); }
uint64_t emu_ji_stream_words_of(uint32_t blocks) { return ji::stream_words_of(blocks); }

// items: n rows of (address, w, h, gray) as u64.  Writes the tables into the caller's arrays (room for n tile records and n + 2
// segment records) and the counts into counts[0..4]: tile records, launches, segment records, passes, blocks.  launches: rows of
// (mode, load, first_record, count, tiles); passes: rows of (mode, first_record, count, groups, blocks, stream_words) as u64.
int emu_ji_build_tables(const uint64_t *items, uint32_t n, int rgb_mode, ji::TileRecord *tiles, uint32_t *tile_item, ji::SegRecord *segs, uint32_t *seg_item,
                        uint32_t *first_group, int *load, uint64_t *launches, uint64_t *passes, uint64_t counts[5])
{
    std::vector<ji::Item> v;
    for (uint32_t k = 0; k < n; ++k) v.push_back({k, items[4 * k], (uint32_t)items[4 * k + 1], (uint32_t)items[4 * k + 2], items[4 * k + 3] != 0});
    ji::Tables t;
    if (!ji::build_tables(v, rgb_mode, t)) return 0;
    std::memcpy(tiles, t.tiles.data(), t.tiles.size() * sizeof(ji::TileRecord));
    std::memcpy(tile_item, t.tile_item.data(), t.tile_item.size() * 4);
    std::memcpy(segs, t.segs.data(), t.segs.size() * sizeof(ji::SegRecord));
    std::memcpy(seg_item, t.seg_item.data(), t.seg_item.size() * 4);
    std::memcpy(first_group, t.first_group.data(), n * 4);
    std::memcpy(load, t.load.data(), n * sizeof(int));
    for (size_t i = 0; i < t.launches.size(); ++i) {
        const ji::CoefLaunch &l = t.launches[i];
        const uint64_t row[5] = {(uint64_t)l.mode, (uint64_t)l.load, l.first_record, l.count, l.tiles};
        std::memcpy(launches + 5 * i, row, sizeof row);
    }
    for (size_t i = 0; i < t.passes.size(); ++i) {
        const ji::CodePass &p = t.passes[i];
        const uint64_t row[6] = {(uint64_t)p.mode, p.first_record, p.count, p.groups, p.blocks, p.stream_words};
        std::memcpy(passes + 6 * i, row, sizeof row);
    }
    counts[0] = t.tiles.size(); counts[1] = t.launches.size(); counts[2] = t.segs.size(); counts[3] = t.passes.size(); counts[4] = t.blocks;
    return 1;
}

} // extern "C"
