// TEST HARNESS: the ragged filter form's host-and-device header (pixo_amd/csrc/png_images_math.h) compiled for the host — the
// row -> image search the kernel runs, the launch class of an image, and the table of a sub-batch as the driver builds it.
#include "../../pixo_amd/csrc/png_images_math.h"

using namespace pixo_png_images;

struct LaunchC { uint32_t cls, bpp, kind, fast, staged, first_record, count, rows, max_row_bytes; };

extern "C" {
uint32_t emu_record_bytes(void) { return (uint32_t)sizeof(Record); }
uint32_t emu_item_bytes(void) { return (uint32_t)sizeof(Item); }
uint32_t emu_image_of_row(const Record *t, uint32_t count, uint32_t y) { return image_of_row(t, count, y); }
int emu_kind_of(int strategy, uint64_t row_bytes) { return kind_of(strategy, row_bytes); }
uint32_t emu_stage_bytes(uint64_t row_bytes) { return stage_bytes(row_bytes); }
uint32_t emu_class_of(uint32_t bpp, int fast, int kind, int staged) { return class_of(bpp, fast != 0, kind, staged != 0); }
int emu_fast_of(uint64_t address, uint64_t row_bytes) { return fast_of(address, row_bytes) ? 1 : 0; }
// -> the number of launches, or -1 when build_table refuses; `table` and `record_item` have room for n entries, `launches` too
int emu_build_table(const Item *items, uint32_t n, uint64_t data_address, Record *table, LaunchC *launches, uint32_t *record_item)
{
    std::vector<Item> in(items, items + n);
    std::vector<Record> t;
    std::vector<Launch> l;
    std::vector<uint32_t> r;
    if (!build_table(in, data_address, t, l, r)) return -1;
    for (size_t i = 0; i < t.size(); ++i) { table[i] = t[i]; record_item[i] = r[i]; }
    for (size_t i = 0; i < l.size(); ++i)
        launches[i] = LaunchC{l[i].cls, l[i].bpp, l[i].kind, l[i].fast ? 1u : 0u, l[i].staged ? 1u : 0u, l[i].first_record, l[i].count, l[i].rows, l[i].max_row_bytes};
    return (int)l.size();
}
}
