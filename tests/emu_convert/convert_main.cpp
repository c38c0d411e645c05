// TEST HARNESS: a stand-alone program that runs the colour conversion's header (pixo_amd/csrc/convert_math.h) on the host —
// the table builder, the tile -> image search against a linear walk, and the lane body of every workgroup of every launch
// over buffers allocated to EXACTLY the images' bytes — so that the host compiler's address and undefined-behaviour
// sanitizers (tests/emu_convert/Makefile) see every load and store the kernels make.  Results are checked against the
// per-pixel functions; the 16-pixel step against them over random groups.
//   convert_main <rounds>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "emu_convert.cpp"

namespace {

struct Held { // an image's two buffers: exactly its bytes, at a chosen residue modulo 16
    void *src_block = nullptr, *dst_block = nullptr;
    uint8_t *src = nullptr, *dst = nullptr;
};
uint8_t *exact(size_t bytes, uint32_t residue, void **block)
{ // the last byte of the image is the last byte of the allocation; the first lies `residue` behind a multiple of 16
    if (posix_memalign(block, 16, bytes + residue)) std::abort();
    return static_cast<uint8_t *>(*block) + residue;
}
template <int KIND> void reference(const uint8_t *s, uint8_t *d, uint64_t pixels, uint32_t bpp)
{
    for (uint64_t p = 0; p < pixels; ++p) convert_pixel<KIND>(s + p * src_bpp(KIND, bpp), d + p * dst_bpp(KIND, bpp), bpp);
}
void reference_of(int kind, const uint8_t *s, uint8_t *d, uint64_t pixels, uint32_t bpp)
{
    switch (kind) {
    case K_COPY: reference<K_COPY>(s, d, pixels, bpp); break;
    case K_GA_G: reference<K_GA_G>(s, d, pixels, bpp); break;
    case K_RGBA_RGB: reference<K_RGBA_RGB>(s, d, pixels, bpp); break;
    case K_RGB_G: reference<K_RGB_G>(s, d, pixels, bpp); break;
    default: reference<K_RGBA_G>(s, d, pixels, bpp); break;
    }
}

} // namespace

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 8;
    std::mt19937_64 rnd(20240611);
    const auto upto = [&](uint64_t n) { return (uint64_t)(rnd() % n); };
    uint64_t images_run = 0, tiles_run = 0;
    for (int round = 0; round < rounds; ++round) {
        const uint32_t n = 1 + (uint32_t)upto(round % 3 == 0 ? 70 : 12);
        static const uint32_t caps[4] = {1, 2, 3, kImageTiles};
        const uint32_t image_tiles = caps[upto(4)];
        std::vector<Item> items(n);
        std::vector<Held> held(n);
        std::vector<std::vector<uint8_t>> want(n);
        for (uint32_t i = 0; i < n; ++i) {
            const int kind = (int)upto(kKinds);
            const uint32_t bpp = kind == K_COPY ? 1 + (uint32_t)upto(4) : src_bpp(kind, 0);
            const uint64_t sizes[8] = {1, 15, 16, 17, kTilePixels - 1, kTilePixels, kTilePixels + 1, 1 + upto(5 * kTilePixels + 40)};
            const uint64_t pixels = sizes[upto(8)];
            const bool aligned = upto(2) == 0;
            const uint32_t rs = aligned ? 0 : (uint32_t)upto(16), rd = aligned ? 0 : (uint32_t)upto(16);
            const size_t in_bytes = pixels * src_bpp(kind, bpp), out_bytes = pixels * dst_bpp(kind, bpp);
            held[i].src = exact(in_bytes, rs, &held[i].src_block);
            held[i].dst = exact(out_bytes, rd, &held[i].dst_block);
            for (size_t b = 0; b < in_bytes; ++b) held[i].src[b] = (uint8_t)rnd();
            std::memset(held[i].dst, 0x5A, out_bytes);
            want[i].resize(out_bytes);
            reference_of(kind, held[i].src, want[i].data(), pixels, bpp);
            items[i] = Item{reinterpret_cast<uint64_t>(held[i].src), reinterpret_cast<uint64_t>(held[i].dst), pixels, (uint32_t)kind, bpp};
        }
        std::vector<Record> table;
        std::vector<Launch> launches;
        std::vector<uint32_t> record_item;
        if (!build_table(items, image_tiles, kMaxTiles, table, launches, record_item)) { std::puts("build_table refused"); return 1; }
        if (table.size() != n || launches.size() > kClasses) { std::puts("table: wrong counts"); return 1; }
        for (const Launch &l : launches) {
            const Record *t = table.data() + l.first_record;
            // the search against a linear walk, for every tile of the launch
            uint32_t tile = 0;
            for (uint32_t r = 0; r < l.count; ++r) {
                const Item &it = items[record_item[l.first_record + r]];
                if (class_of((int)it.kind, form_of(it.src, it.dst)) != l.cls || t[r].first_tile != tile || t[r].tiles != tiles_of(it.pixels, image_tiles)) {
                    std::puts("table: a record is not its item's");
                    return 1;
                }
                for (uint32_t k = 0; k < t[r].tiles; ++k, ++tile)
                    if (image_of_tile(t, l.count, tile) != r) { std::printf("search: tile %u is not in record %u\n", tile, r); return 1; }
            }
            if (tile != l.tiles) { std::puts("table: a launch's tiles are not its records' summed"); return 1; }
            if (run_launch(t, l.count, l.tiles, (int)(l.cls / kForms), (int)(l.cls % kForms))) { std::puts("a tile outside its image"); return 1; }
            tiles_run += l.tiles;
        }
        for (uint32_t i = 0; i < n; ++i) {
            if (std::memcmp(held[i].dst, want[i].data(), want[i].size())) { std::printf("round %d: image %u differs from the per-pixel functions\n", round, i); return 1; }
            std::free(held[i].src_block);
            std::free(held[i].dst_block);
        }
        images_run += n;
    }
    // the 16-pixel step against the per-pixel functions, over random groups
    for (int kind = K_GA_G; kind <= K_RGBA_G; ++kind) {
        const uint32_t groups = 257, sb = src_bpp(kind, 0), db = dst_bpp(kind, 0);
        std::vector<uint8_t> in(groups * 16 * sb), out(groups * 16 * db), want(groups * 16 * db);
        for (uint8_t &b : in) b = (uint8_t)rnd();
        emu_cv_convert16(kind, in.data(), out.data(), groups);
        reference_of(kind, in.data(), want.data(), groups * 16, 0);
        if (out != want) { std::printf("convert16: kind %d differs\n", kind); return 1; }
    }
#if defined(PIXO_SANITIZED)
    const char *how = "address + undefined-behaviour sanitizers";
#else
    const char *how = "no sanitizer runtime on this machine: plain";
#endif
    std::printf("convert_main ok: %llu images, %llu tiles (%s)\n", (unsigned long long)images_run, (unsigned long long)tiles_run, how);
    return 0;
}
