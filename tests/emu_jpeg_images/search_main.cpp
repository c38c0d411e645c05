// TEST HARNESS: a stand-alone program (its own main; built with -fsanitize=address,undefined where the runtime is installed)
// that runs the ragged JPEG form's searches (pixo_amd/csrc/jpeg_images_math.h) over random tables held in exactly sized heap
// arrays — a search that reads one record too far, or a table whose offsets overflow, ends the program — and holds every
// answer against a linear scan.  search_main [rounds]; prints "search_main ok ..." and returns 0.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../../pixo_amd/csrc/jpeg_images_math.h"

namespace ji = pixo_jpeg_images;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

static int fail(const char *what, uint32_t a, uint32_t b, uint32_t c)
{
    std::printf("search_main FAILED: %s (%u, %u, %u)\n", what, a, b, c);
    return 1;
}

// One table of `count` images: random sizes (1 tile and many), searched at the first and last tile / group of every image and at
// random ones in between
static int one_table(uint32_t count, int rgb_mode, uint32_t max_side)
{
    std::vector<ji::Item> items;
    uint64_t at = rnd(16);
    for (uint32_t k = 0; k < count; ++k) {
        const bool gray = rnd(2) == 0;
        const uint32_t w = 1 + rnd(max_side), h = 1 + rnd(rnd(4) ? 24 : max_side);
        items.push_back({k, at, w, h, gray});
        at += (uint64_t)w * h * (gray ? 1 : 3) + rnd(5);
    }
    ji::Tables t;
    if (!ji::build_tables(items, rgb_mode, t)) return fail("build_tables", count, 0, 0);
    for (const ji::CoefLaunch &l : t.launches) {
        // (an exactly sized copy: the sanitizer sees a read beyond the launch's records)
        std::unique_ptr<ji::TileRecord[]> table(new ji::TileRecord[l.count]);
        for (uint32_t r = 0; r < l.count; ++r) table[r] = t.tiles[l.first_record + r];
        uint32_t tile = 0;
        for (uint32_t r = 0; r < l.count; ++r) {
            const ji::Shape s = ji::shape_of(l.mode, table[r].wh & 0xFFFFu, table[r].wh >> 16);
            const uint32_t tiles = s.tiles_x * s.tiles_y;
            if (table[r].first_tile != tile || tiles == 0 || table[r].tiles_x != s.tiles_x) return fail("first_tile", r, table[r].first_tile, tile);
            const uint32_t probes[3] = {tile, tile + tiles - 1, tile + rnd(tiles)};
            for (uint32_t p : probes)
                if (ji::image_of_tile(table.get(), l.count, p) != r) return fail("image_of_tile", p, r, l.count);
            tile += tiles;
        }
        if (tile != l.tiles) return fail("tiles", tile, l.tiles, 0);
    }
    for (const ji::CodePass &p : t.passes) {
        std::unique_ptr<ji::SegRecord[]> table(new ji::SegRecord[p.count + 1]);
        for (uint32_t r = 0; r <= p.count; ++r) table[r] = t.segs[p.first_record + r];
        uint32_t group = 0;
        for (uint32_t r = 0; r < p.count; ++r) {
            const uint32_t groups = ji::groups_of(table[r].blocks);
            if (table[r].first_group != group || groups == 0) return fail("first_group", r, table[r].first_group, group);
            const uint32_t probes[3] = {group, group + groups - 1, group + rnd(groups)};
            for (uint32_t g : probes)
                if (ji::segment_of_group(table.get(), p.count, g) != r) return fail("segment_of_group", g, r, p.count);
            group += groups;
        }
        if (group != p.groups || table[p.count].first_group != p.groups) return fail("groups", group, p.groups, 0);
    }
    return 0;
}

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 20;
    for (int r = 0; r < rounds; ++r) {
        const uint32_t counts[5] = {1, 2, 3, 1 + rnd(40), 1 + rnd(400)};
        for (uint32_t count : counts)
            for (int mode = 0; mode < 2; ++mode)
                if (one_table(count, mode, r % 3 == 0 ? 2000 : 200)) return 1;
    }
    if (one_table(65535, ji::MODE_420, 40)) return 1; // the largest batch
#if defined(PIXO_SANITIZED)
    std::printf("search_main ok (%d rounds, address + undefined sanitizers)\n", rounds);
#else
    std::printf("search_main ok (%d rounds, no sanitizer runtime on this host)\n", rounds);
#endif
    return 0;
}
