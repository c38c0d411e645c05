// resize_images_math.h — the ragged form of the resize kernels (resize.hip, *_images_kernel): sources of individual sizes and
// bytes per pixel to destinations of individual sizes, in one flat launch per pass.  The record a workgroup reads, the tile ->
// (image, tile x, tile y) search, the tiles of an image per pass and the table of a sub-batch.  Compiled for gfx950 by
// resize.hip and for the HOST by the driver (resize_api.cpp), the plan entry and tests/emu_resize_images: kernel, driver and
// plan run the same search and the same counts.  No HIP headers in here.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define PIXO_RZI_HD __host__ __device__ inline
#else
#define PIXO_RZI_HD inline
#endif

namespace pixo_resize_images {

// One image of one pass of a ragged launch: everything the single entry's kernel arguments hold once.  A launch is a flat
// 1-D grid over all tiles of its images; an image's tiles are numbered row of tiles after row of tiles from first_tile.
struct Record {
    uint64_t src;        // the address of the image's first source byte, any alignment
    uint64_t dst;        // ... of its first destination byte, any alignment
    uint64_t mid_at;     // Lanczos3: where its sh rows of the intermediate start, from the sub-batch's block (a multiple of 16)
    uint64_t mid_stride; // ... the bytes of one of those rows: dw * bpp rounded up to 16
    uint64_t h_at, v_at; // ... its horizontal (sw -> dw) and vertical (sh -> dh) axis in the block of tables
    uint32_t sw, sh, dw, dh;
    uint32_t bpp;        // bytes per pixel, 1..4
    uint32_t use_lds;    // Lanczos3: the horizontal pass stages this image's tiles in LDS
    uint32_t first_tile; // its first tile in the launch: the tiles of the records in front of it summed
    uint32_t tiles_x;    // tiles per row of tiles
    uint32_t tiles_y;    // rows of tiles; a workgroup strides over the image's rows in steps of tiles_y * (rows per tile)
    uint32_t reserved;
};
static_assert(sizeof(Record) == 88, "uploaded as it is");

// The passes and what one tile (one workgroup) of each covers
enum { PASS_POINT = 0, PASS_H = 1, PASS_V = 2 };
constexpr uint32_t kPointTileCols = 256, kPointTileRows = 4; // nearest / bilinear: destination columns x destination rows
constexpr uint32_t kHTileCols = 64, kHTileRows = 4;          // Lanczos3 horizontal: destination columns x SOURCE rows
constexpr uint32_t kVTileBytes = 1024, kVTileRows = 1;       // Lanczos3 vertical: bytes of a destination row x destination rows
constexpr uint32_t kRowsCap = 65535;                         // rows of tiles an image has at most (the single entry's grid.y limit)
constexpr uint64_t kMaxTiles = 0x7FFFFFFFull;                // tiles of one launch at most

// The image that holds tile t of the launch: the last record whose first_tile is not behind t.  count >= 1, first_tile[0] ==
// 0, strictly ascending (every image has a tile).  Table: a pointer to records (the kernels pass one into the constant
// address space: t is uniform across a workgroup, so the loads are scalar ones).
template <class Table> PIXO_RZI_HD uint32_t image_of_tile(Table t, uint32_t count, uint32_t tile)
{
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (t[mid].first_tile <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}
// ... and the tile's place in that image (tile - first_tile, row of tiles after row of tiles)
PIXO_RZI_HD void tile_in_image(uint32_t tile, uint32_t first_tile, uint32_t tiles_x, uint32_t *tx, uint32_t *ty)
{
    const uint32_t t = tile - first_tile;
    *tx = t % tiles_x;
    *ty = t / tiles_x;
}

// The tiles of one image in one pass.  rows_cap (1..kRowsCap) bounds the rows of tiles; what does not fit is reached by the
// kernels' row-stride loops.  An image whose tiles alone would exceed kMaxTiles gets fewer rows of tiles still.
PIXO_RZI_HD void tiles_of(int pass, uint32_t sh, uint32_t dw, uint32_t dh, uint32_t bpp, uint32_t rows_cap, uint32_t *tiles_x, uint32_t *tiles_y)
{
    uint64_t across, rows;
    if (pass == PASS_POINT) { across = ((uint64_t)dw + kPointTileCols - 1) / kPointTileCols; rows = ((uint64_t)dh + kPointTileRows - 1) / kPointTileRows; }
    else if (pass == PASS_H) { across = ((uint64_t)dw + kHTileCols - 1) / kHTileCols; rows = ((uint64_t)sh + kHTileRows - 1) / kHTileRows; }
    else { across = ((uint64_t)dw * bpp + kVTileBytes - 1) / kVTileBytes; rows = ((uint64_t)dh + kVTileRows - 1) / kVTileRows; }
    if (rows > rows_cap) rows = rows_cap;
    if (rows > kMaxTiles / across) rows = kMaxTiles / across; // (across <= 2^18: at least 8191 rows of tiles stay)
    *tiles_x = (uint32_t)across;
    *tiles_y = (uint32_t)rows;
}
PIXO_RZI_HD uint64_t tile_count(int pass, uint32_t sh, uint32_t dw, uint32_t dh, uint32_t bpp, uint32_t rows_cap)
{
    uint32_t tx, ty;
    tiles_of(pass, sh, dw, dh, bpp, rows_cap, &tx, &ty);
    return (uint64_t)tx * ty;
}

// ---- host: the table of one pass of a sub-batch ------------------------------------------------------------------------
// One image of the sub-batch, in index order: a Record without its place in a launch.
struct Item {
    uint64_t src, dst, mid_at, mid_stride, h_at, v_at;
    uint32_t sw, sh, dw, dh, bpp, use_lds;
};
struct Launch {
    uint32_t bpp;                 // the launch's bytes per pixel; 0: the vertical pass, which is byte-wise (all images in one launch)
    uint32_t first_record, count; // its records in the table
    uint32_t tiles;               // their tiles summed: the grid
};
// items (index order) -> the records of `pass`, grouped by bytes per pixel (ascending, index order inside a group; PASS_V: one
// group in index order), and one Launch per group.  record_item[r]: the item record r describes.  False: the tiles of a
// launch do not fit 31 bits (the driver ends a sub-batch before that).
inline bool build_table(const std::vector<Item> &items, int pass, uint32_t rows_cap, std::vector<Record> &table, std::vector<Launch> &launches,
                        std::vector<uint32_t> &record_item)
{
    const uint32_t n = (uint32_t)items.size();
    std::vector<uint32_t> order(n);
    for (uint32_t k = 0; k < n; ++k) order[k] = k;
    if (pass != PASS_V) std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return items[a].bpp < items[b].bpp; });
    table.clear(); launches.clear(); record_item.clear();
    for (uint32_t r = 0; r < n; ++r) {
        const uint32_t k = order[r];
        const Item &it = items[k];
        const uint32_t group = pass == PASS_V ? 0u : it.bpp;
        if (launches.empty() || launches.back().bpp != group) launches.push_back(Launch{group, r, 0, 0});
        Launch &l = launches.back();
        uint32_t tx, ty;
        tiles_of(pass, it.sh, it.dw, it.dh, it.bpp, rows_cap, &tx, &ty);
        if ((uint64_t)l.tiles + (uint64_t)tx * ty > kMaxTiles) return false;
        table.push_back(Record{it.src, it.dst, it.mid_at, it.mid_stride, it.h_at, it.v_at, it.sw, it.sh, it.dw, it.dh, it.bpp, it.use_lds, l.tiles, tx, ty, 0});
        record_item.push_back(k);
        l.tiles += tx * ty;
        l.count += 1;
    }
    return true;
}

} // namespace pixo_resize_images
