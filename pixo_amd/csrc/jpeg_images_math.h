// jpeg_images_math.h — JPEG encode of images of individual sizes (jpeg_images.hip, jpeg_images_api.cpp): the record a tile of the
// ragged coefficient kernel reads, the record a group of the ragged coding pass reads, the two searches, the class of an image
// and the table of a sub-batch.  Compiled for gfx950 by jpeg_images.hip and jpeg_scan_fused.hip and for the HOST by the driver, the
// plan entry and tests/emu_jpeg_images: kernels, driver and plan run the same searches and the same counts.  No HIP headers in here.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define PIXO_JI_HD __host__ __device__ inline
#else
#define PIXO_JI_HD inline
#endif

namespace pixo_jpeg_images {

// The block order of an image (pixo_tile::Mode, jpeg_tile.h) and how its tiles read their pixels (pixo_tile::Load)
enum { MODE_420 = 0, MODE_444 = 1, MODE_GRAY = 2 };
enum { LOAD_BYTES = 0, LOAD_ALIGNED = 1, LOAD_FUNNEL = 2 };
constexpr uint32_t kGroupBlocks = 192; // blocks a group of the coding pass holds (jpeg_scan_dev.h kGroup)

// One image of one ragged coefficient launch (one mode, one load form).  The launch is a flat 1-D grid over the tiles of its
// images; an image's tiles are numbered row of tiles after row of tiles from first_tile.  Sides are at most 65535: two to a word.
struct TileRecord {
    uint64_t px;         // the address of the image's first pixel byte, any alignment
    uint32_t first_tile; // its first tile in the launch: the tiles of the records in front of it summed
    uint32_t wh;         // W | H << 16
    uint32_t units;      // units_x | units_y << 16: MCUs (4:2:0) or 8x8 blocks a row / rows of them (at most 8192 each)
    uint32_t tiles_x;    // tiles per row of tiles
    uint32_t y_block, cb_block, cr_block; // where its Y, Cb and Cr planes begin in the sub-batch's tuple, in blocks of 64 coefficients
    uint32_t reserved;
};
static_assert(sizeof(TileRecord) == 40, "uploaded as it is");

// One image (a byte-aligned segment) of one coding pass (one colour class).  A pass is a flat grid over the groups of 192
// blocks of its segments; a table of n segments has n + 1 records, the last one holds the pass's group count in first_group.
struct SegRecord {
    uint32_t first_group; // its first group in the pass: the look-back's floor
    uint32_t blocks;      // its blocks in scan order
    uint32_t y_block, cb_block, cr_block; // as in its TileRecord
    uint32_t reserved;
    uint64_t stream_word; // where its packed stream begins in the pass's stream buffer (32-bit words; a multiple of 4)
};
static_assert(sizeof(SegRecord) == 32, "uploaded as it is");

// The record that holds tile t (group g): the last one whose first_tile (first_group) is not behind it.  count >= 1, the first
// record starts at 0, strictly ascending (every image has a tile and a group).  Table: a pointer to records — the kernels pass
// one into the constant address space: t is uniform across a workgroup, so the search's loads are scalar ones.
template <class Table> PIXO_JI_HD uint32_t image_of_tile(Table t, uint32_t count, uint32_t tile)
{
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (t[mid].first_tile <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}
template <class Table> PIXO_JI_HD uint32_t segment_of_group(Table t, uint32_t count, uint32_t group)
{
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (t[mid].first_group <= group) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- an image's geometry and class -------------------------------------------------------------------------------------------
struct Shape {
    uint32_t units_x, units_y, tiles_x, tiles_y;
    uint32_t y_blocks, c_blocks; // blocks of the Y plane, of each chroma plane (gray: 0)
};
PIXO_JI_HD Shape shape_of(int mode, uint32_t w, uint32_t h)
{
    const uint32_t unit = mode == MODE_420 ? 16u : 8u, per_tile = mode == MODE_420 ? 32u : 64u, tile_h = mode == MODE_420 ? 16u : (mode == MODE_444 ? 8u : 24u);
    Shape s;
    s.units_x = (w + unit - 1) / unit;
    s.units_y = (h + unit - 1) / unit;
    s.tiles_x = (s.units_x + per_tile - 1) / per_tile;
    s.tiles_y = (s.units_y * unit + tile_h - 1) / tile_h;
    const uint32_t units = s.units_x * s.units_y; // (at most 4096 x 4096 for 4:2:0, 8192 x 8192 otherwise: 32 bits hold the blocks)
    s.y_blocks = mode == MODE_420 ? 4 * units : units;
    s.c_blocks = mode == MODE_GRAY ? 0 : units;
    return s;
}
PIXO_JI_HD uint32_t blocks_of(const Shape &s) { return s.y_blocks + 2 * s.c_blocks; }
PIXO_JI_HD uint32_t groups_of(uint32_t blocks) { return (blocks + kGroupBlocks - 1) / kGroupBlocks; }
// The load form of an image from its first byte's address and its row length (jpeg_kernels.hip launch_jpeg_coeffs, one image):
// narrower than one 4-pixel group: byte gathers; every row dword aligned: 12-byte loads; otherwise loads at the lane's own address.
PIXO_JI_HD int load_form_of(uint64_t address, uint32_t w, uint32_t bpp)
{
    if (w < 4) return LOAD_BYTES;
    return (address % 4 == 0 && ((uint64_t)w * bpp) % 4 == 0) ? LOAD_ALIGNED : LOAD_FUNNEL;
}
// (the plan entry's numbering: 0 aligned, 1 funnel, 2 bytes)
PIXO_JI_HD uint8_t plan_load_form(int load) { return load == LOAD_ALIGNED ? 0 : (load == LOAD_FUNNEL ? 1 : 2); }
// The words of a segment's packed stream: a block has at most 1665 bits (209 bytes), + 64 bytes the kernels read into, a multiple of 16 bytes
PIXO_JI_HD uint64_t stream_words_of(uint32_t blocks) { return ((uint64_t)blocks * 209 + 64 + 15) / 16 * 4; }

// ---- host: the tables of a sub-batch --------------------------------------------------------------------------------------------
// A sub-batch holds at most this many blocks (debug switch jpeg_images_blocks lowers it): 512 MiB of tuple at 128 bytes a block and
// 836 MiB of packed streams at 209 — what the context's buffers hold for a batch of 85 images of 1920x1080 at 4:2:0 today.
constexpr uint64_t kSubBatchBlocks = uint64_t{1} << 22;

struct Item { // one image of a sub-batch that goes the shared way, in index order
    uint32_t image;   // its index in the sub-batch
    uint64_t address; // of its first pixel byte
    uint32_t w, h;
    bool gray;
};
struct CoefLaunch { // one ragged coefficient launch: a class (mode x load form) present in the sub-batch
    int mode, load;
    uint32_t first_record, count, tiles;
};
struct CodePass { // one coding pass + one stuffing pass: a colour class present in the sub-batch
    int mode;
    uint32_t first_record, count; // count segments, count + 1 records
    uint32_t groups;
    uint64_t blocks, stream_words;
};
struct Tables {
    std::vector<TileRecord> tiles;
    std::vector<CoefLaunch> launches;  // gray before RGB, load forms ascending, index order inside a class
    std::vector<uint32_t> tile_item;   // the item tile record r describes
    std::vector<SegRecord> segs;
    std::vector<CodePass> passes;      // gray before RGB, index order inside a pass
    std::vector<uint32_t> seg_item;    // the item segment record r describes (a pass's last record: ~0)
    std::vector<uint32_t> first_group; // per item: its first group in its pass
    std::vector<int> load;             // per item: its load form
    uint64_t blocks = 0;               // of the whole tuple
};
// rgb_mode: MODE_420 or MODE_444, the template's subsampling.  False: tiles, groups or blocks of a launch do not fit 31 bits
// (the driver ends a sub-batch long before that).
inline bool build_tables(const std::vector<Item> &items, int rgb_mode, Tables &t)
{
    const uint32_t n = (uint32_t)items.size();
    t = Tables{};
    t.first_group.assign(n, 0);
    t.load.assign(n, 0);
    std::vector<Shape> shape(n);
    std::vector<uint32_t> y_at(n);
    uint64_t at = 0;
    for (uint32_t k = 0; k < n; ++k) { // the tuple: image after image, each one's Y, Cb, Cr planes back to back
        const Item &it = items[k];
        shape[k] = shape_of(it.gray ? MODE_GRAY : rgb_mode, it.w, it.h);
        t.load[k] = load_form_of(it.address, it.w, it.gray ? 1u : 3u);
        if (at + blocks_of(shape[k]) > 0x7FFFFFFFull) return false;
        y_at[k] = (uint32_t)at;
        at += blocks_of(shape[k]);
    }
    t.blocks = at;
    for (int colour = 0; colour < 2; ++colour) {
        const int mode = colour == 0 ? MODE_GRAY : rgb_mode;
        for (int load = 0; load < 3; ++load) {
            CoefLaunch l{mode, load, (uint32_t)t.tiles.size(), 0, 0};
            for (uint32_t k = 0; k < n; ++k) {
                if (items[k].gray != (colour == 0) || t.load[k] != load) continue;
                const Shape &s = shape[k];
                const uint64_t tiles = (uint64_t)s.tiles_x * s.tiles_y;
                if (l.tiles + tiles > 0x7FFFFFFFull) return false;
                t.tiles.push_back(TileRecord{items[k].address, l.tiles, items[k].w | items[k].h << 16, s.units_x | s.units_y << 16, s.tiles_x, y_at[k],
                                             y_at[k] + s.y_blocks, y_at[k] + s.y_blocks + s.c_blocks, 0});
                t.tile_item.push_back(k);
                l.tiles += (uint32_t)tiles;
                l.count += 1;
            }
            if (l.count) t.launches.push_back(l);
        }
        CodePass p{mode, (uint32_t)t.segs.size(), 0, 0, 0, 0};
        for (uint32_t k = 0; k < n; ++k) {
            if (items[k].gray != (colour == 0)) continue;
            const Shape &s = shape[k];
            const uint32_t blocks = blocks_of(s);
            if ((uint64_t)p.groups + groups_of(blocks) > 0x7FFFFFFFull) return false;
            t.segs.push_back(SegRecord{p.groups, blocks, y_at[k], y_at[k] + s.y_blocks, y_at[k] + s.y_blocks + s.c_blocks, 0, p.stream_words});
            t.seg_item.push_back(k);
            t.first_group[k] = p.groups;
            p.groups += groups_of(blocks);
            p.blocks += blocks;
            p.stream_words += stream_words_of(blocks);
            p.count += 1;
        }
        if (p.count) {
            t.segs.push_back(SegRecord{p.groups, 0, 0, 0, 0, 0, p.stream_words});
            t.seg_item.push_back(~0u);
            t.passes.push_back(p);
        }
    }
    return true;
}

} // namespace pixo_jpeg_images
