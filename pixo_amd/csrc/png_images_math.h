// png_images_math.h — the ragged form of the PNG filter kernels (png_filter.hip, MODE == RAGGED): images of individual
// widths, heights and bytes per pixel in one launch.  The record a workgroup reads, the row -> image search, the launch
// class of an image and the table of a sub-batch.  Compiled for gfx950 by png_filter.hip and for the HOST by the driver
// (png_api.cpp), the plan entry and tests/emu_png_images: kernel, driver and plan run the same search and the same choice.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define PIXO_IMG_HD __host__ __device__ inline
#else
#define PIXO_IMG_HD inline
#endif

namespace pixo_png_images {

// One image of a ragged launch.  Everything a workgroup needs that the single image's Args hold once.
struct Record {
    uint64_t src;       // the image's first byte, counted from the launch's data pointer
    uint64_t dst;       // its filtered stream's first byte, counted from the launch's output pointer
    uint64_t sums_at;   // its first row's index into row_sums ([2] each)
    uint32_t row_bytes; // width * bytes per pixel
    uint32_t height;
    uint32_t first_row; // its first row in the launch: the heights in front of it summed
    int32_t strategy;   // what png_plan resolved for it
};

// The image that holds row y of the launch: the last record whose first_row is not behind y.  count >= 1, first_row[0] == 0,
// strictly ascending (every image has a row).  Table: a pointer to records (the kernel passes one into the constant address
// space: y is uniform across a workgroup, so the loads are scalar ones).
template <class Table> PIXO_IMG_HD uint32_t image_of_row(Table t, uint32_t count, uint32_t y)
{
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (t[mid].first_row <= y) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The kernel forms, as png_filter.hip's launch_bpp chooses them (K_GENERAL .. K_REGS512 are the kernel's KIND; the register
// form of Bigrams is a kernel of its own).
enum { KIND_GENERAL = 0, KIND_REGS = 1, KIND_BIGRAMS = 2, KIND_REGS512 = 3, KIND_BIGRAMS_REGS = 4, KINDS = 5 };
constexpr int kStrategyPaeth = 4, kStrategyBigrams = 8;     // (png_filter.hpp PNG_S_PAETH, PNG_S_BIGRAMS)
constexpr uint64_t kRegDwords = 4 * 256 * 4;                // dwords of a row 256 threads hold: kRegIters * kThreads * 4
constexpr uint64_t kStageLimit = 48 * 1024;

// Dynamic LDS of the staged write-out: 16 bytes in front (filter byte at 15), the row in whole 16-byte groups, 32 bytes of
// slack for the fifth dword of the last chunk.  0: the row is too long, its bytes are stored directly.
PIXO_IMG_HD uint32_t stage_bytes(uint64_t row_bytes)
{
    const uint64_t stage = 16 + ((row_bytes + 15) & ~15ull) + 32;
    return stage <= kStageLimit ? (uint32_t)stage : 0u;
}
PIXO_IMG_HD int kind_of(int strategy, uint64_t row_bytes)
{
    const uint64_t ndw = (row_bytes + 3) / 4;
    const bool staged = stage_bytes(row_bytes) != 0;
    if (strategy == kStrategyBigrams) return staged && ndw <= kRegDwords ? KIND_BIGRAMS_REGS : KIND_BIGRAMS;
    if (strategy > kStrategyPaeth && staged && ndw <= 2 * kRegDwords) return ndw <= kRegDwords ? KIND_REGS : KIND_REGS512;
    return KIND_GENERAL;
}
// Images of one class share a launch: bytes per pixel (1..4), aligned loads (the image's first byte and its row length are
// multiples of 4), the kernel form, and whether the rows are staged in LDS — rows past the stage are a class of their own,
// so that "staged" stays one decision per launch as in the single-image form.
PIXO_IMG_HD uint32_t class_of(uint32_t bpp, bool fast, int kind, bool staged)
{
    return (((bpp - 1) * 2 + (fast ? 1u : 0u)) * KINDS + (uint32_t)kind) * 2 + (staged ? 1u : 0u);
}
PIXO_IMG_HD bool fast_of(uint64_t address, uint64_t row_bytes) { return address % 4 == 0 && row_bytes % 4 == 0; }

// ---- host: the table of a sub-batch ----------------------------------------------------------------------------------
// One image that takes the batched way in, in index order.
struct Item {
    uint32_t image;     // its index in the sub-batch
    uint64_t src, dst;  // as Record
    uint32_t row_bytes, height, bpp;
    int32_t strategy;
};
struct Launch {
    uint32_t cls, bpp, kind;
    bool fast, staged;
    uint32_t first_record, count, rows; // its records in the table, their rows summed
    uint32_t max_row_bytes;             // the class's longest row: what the dynamic LDS is sized for
};
// items (index order) -> the records grouped by class (classes ascending, index order inside a class) and one Launch per
// class present.  sums_at follows INDEX order over the items, whatever the class: image k's sums lie behind those of the
// items in front of it.  record_item[r]: the item record r describes.  data_address: where src counts from.  False: the
// rows of a launch do not fit 31 bits.
inline bool build_table(const std::vector<Item> &items, uint64_t data_address, std::vector<Record> &table, std::vector<Launch> &launches,
                        std::vector<uint32_t> &record_item)
{
    const uint32_t n = (uint32_t)items.size();
    std::vector<uint32_t> cls(n), order(n);
    std::vector<uint64_t> sums_at(n);
    uint64_t rows = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const Item &it = items[k];
        const int kind = kind_of(it.strategy, it.row_bytes);
        cls[k] = class_of(it.bpp, fast_of(data_address + it.src, it.row_bytes), kind, stage_bytes(it.row_bytes) != 0);
        order[k] = k;
        sums_at[k] = rows;
        rows += it.height;
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cls[a] < cls[b]; });
    table.clear(); launches.clear(); record_item.clear();
    for (uint32_t r = 0; r < n; ++r) {
        const uint32_t k = order[r];
        const Item &it = items[k];
        if (launches.empty() || launches.back().cls != cls[k]) {
            Launch l{};
            l.cls = cls[k];
            l.bpp = it.bpp;
            l.kind = (uint32_t)kind_of(it.strategy, it.row_bytes);
            l.fast = fast_of(data_address + it.src, it.row_bytes);
            l.staged = stage_bytes(it.row_bytes) != 0;
            l.first_record = r;
            launches.push_back(l);
        }
        Launch &l = launches.back();
        if ((uint64_t)l.rows + it.height > 0x7FFFFFFFull) return false;
        table.push_back(Record{it.src, it.dst, sums_at[k], it.row_bytes, it.height, l.rows, it.strategy});
        record_item.push_back(k);
        l.rows += it.height;
        l.count += 1;
        l.max_row_bytes = std::max(l.max_row_bytes, it.row_bytes);
    }
    return true;
}

} // namespace pixo_png_images
