// convert_math.h — colour conversion (convert.hip): the five conversions the reference's front end makes before it encodes
// (src/bin/pixo.rs:478-513: to_grayscale, rgba_to_rgb, gray_alpha_to_gray), their per-pixel and 16-pixel forms, the whole
// body a lane of the kernels runs, and the ragged launch: the record a workgroup reads, the tile -> image search, the tiles
// of an image and the table of a sub-batch.  Compiled for gfx950 by convert.hip and for the HOST by the driver
// (convert_api.cpp), the plan entry and tests/emu_convert: kernel, driver, plan and emulation run the same code.  No HIP
// headers in here.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define PIXO_CV_HD __host__ __device__ inline
#else
#define PIXO_CV_HD inline
#endif

namespace pixo_convert {

// ---- kinds ------------------------------------------------------------------------------------------------------------------
// Colour types as include/pixo_hip.h: 0 Gray, 1 GrayAlpha, 2 Rgb, 3 Rgba; bytes per pixel = type + 1.
enum { K_COPY = 0, K_GA_G = 1, K_RGBA_RGB = 2, K_RGB_G = 3, K_RGBA_G = 4, kKinds = 5, K_NONE = -1 };
enum { F_ALIGNED = 0, F_BYTES = 1, kForms = 2 };
enum { T_OPAQUE = 0, T_GRAY = 1 }; // PIXO_CONVERT_OPAQUE, PIXO_CONVERT_GRAY
constexpr uint32_t kClasses = kKinds * kForms;
constexpr uint32_t kMaxSide = 1u << 24;

// The pairs the reference has a function for; every other pair (Gray -> Rgb, anything that adds alpha, ...) is K_NONE.
PIXO_CV_HD int kind_of(uint32_t src_ct, uint32_t dst_ct)
{
    if (src_ct > 3 || dst_ct > 3) return K_NONE;
    if (src_ct == dst_ct) return K_COPY;
    if (src_ct == 1 && dst_ct == 0) return K_GA_G;
    if (src_ct == 3 && dst_ct == 2) return K_RGBA_RGB;
    if (src_ct == 2 && dst_ct == 0) return K_RGB_G;
    if (src_ct == 3 && dst_ct == 0) return K_RGBA_G;
    return K_NONE;
}
// The colour type `target` gives a source of src_ct (0..3); -1: an unknown target.  OPAQUE is what the reference does in
// front of a JPEG (pixo.rs:619-638), GRAY its --grayscale.
PIXO_CV_HD int target_type(uint32_t target, uint32_t src_ct)
{
    if (target == T_GRAY) return 0;
    if (target == T_OPAQUE) return src_ct == 1 ? 0 : src_ct == 3 ? 2 : (int)src_ct;
    return -1;
}
// Bytes per pixel of a kind's two sides (K_COPY: the image's own, `bpp`)
PIXO_CV_HD constexpr uint32_t src_bpp(int kind, uint32_t bpp) { return kind == K_GA_G ? 2u : kind == K_RGB_G ? 3u : kind == K_COPY ? bpp : 4u; }
PIXO_CV_HD constexpr uint32_t dst_bpp(int kind, uint32_t bpp) { return kind == K_RGBA_RGB ? 3u : kind == K_COPY ? bpp : 1u; }

// ---- per pixel --------------------------------------------------------------------------------------------------------------
PIXO_CV_HD uint32_t luma(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; } // pixo.rs:489 (at most 255)
// One pixel at s -> one pixel at d
template <int KIND> PIXO_CV_HD void convert_pixel(const uint8_t *s, uint8_t *d, uint32_t bpp)
{
    if (KIND == K_COPY) { for (uint32_t k = 0; k < bpp; ++k) d[k] = s[k]; }
    else if (KIND == K_GA_G) d[0] = s[0];
    else if (KIND == K_RGBA_RGB) { d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; }
    else d[0] = (uint8_t)luma(s[0], s[1], s[2]);
}
// Sixteen pixels held in dwords (little endian: byte i of the run is bits 8 * (i % 4) of word i / 4): 4 * source-bpp words in,
// 4 * destination-bpp words out.  Fully unrolled: the arrays stay in registers.  Not for K_COPY (whole words move).
PIXO_CV_HD uint32_t byte_of(const uint32_t *w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }
template <int KIND> PIXO_CV_HD void convert16(const uint32_t *in, uint32_t *out)
{
    constexpr int sb = (int)src_bpp(KIND, 0), db = (int)dst_bpp(KIND, 0);
#pragma unroll
    for (int w = 0; w < 4 * db; ++w) out[w] = 0;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        if (KIND == K_RGB_G || KIND == K_RGBA_G) {
            out[p >> 2] |= luma(byte_of(in, p * sb), byte_of(in, p * sb + 1), byte_of(in, p * sb + 2)) << (8 * (p & 3));
        } else {
#pragma unroll
            for (int c = 0; c < db; ++c) out[(p * db + c) >> 2] |= byte_of(in, p * sb + c) << (8 * ((p * db + c) & 3));
        }
    }
}

// ---- what a lane does ---------------------------------------------------------------------------------------------------------
// An image is a flat run of `pixels` pixels; a tile is kTilePixels consecutive ones, 16 per lane of a kWorkgroup-lane
// workgroup.  An image has at most kImageTiles tiles: its workgroups stride over what is left.
constexpr uint32_t kWorkgroup = 256;
constexpr uint32_t kLanePixels = 16;
constexpr uint32_t kTilePixels = kWorkgroup * kLanePixels; // 4096
constexpr uint32_t kImageTiles = 65536;
constexpr uint64_t kMaxTiles = 0x7FFFFFFFull; // tiles of one launch at most

typedef uint32_t Quad __attribute__((ext_vector_type(4))); // one dwordx4 load or store
// (PIXO_CV_NT: measurement builds only — bit 0 non-temporal loads, bit 1 non-temporal stores)
PIXO_CV_HD Quad load_quad(const uint8_t *p, uint64_t k)
{
#if defined(PIXO_CV_NT) && (PIXO_CV_NT & 1)
    return __builtin_nontemporal_load(reinterpret_cast<const Quad *>(p) + k);
#else
    return reinterpret_cast<const Quad *>(p)[k];
#endif
}
PIXO_CV_HD void store_quad(uint8_t *p, uint64_t k, Quad q)
{
#if defined(PIXO_CV_NT) && (PIXO_CV_NT & 2)
    __builtin_nontemporal_store(q, reinterpret_cast<Quad *>(p) + k);
#else
    reinterpret_cast<Quad *>(p)[k] = q;
#endif
}

// Lane `lane` of the workgroup that runs tile `tile` of an image of `tiles` tiles.  F_ALIGNED: src and dst are multiples of
// 16, so every whole group of 16 pixels moves in dwordx4 loads and stores; the image's last pixels % 16 go pixel by pixel
// (K_COPY: the same bytes of the tile, dealt to the lanes quad by quad instead of 16 pixels each — below).
// F_BYTES: every pixel goes by itself.  Reads only [src, src + pixels * source-bpp), writes only [dst, dst + pixels * destination-bpp).
template <int KIND, int FORM>
PIXO_CV_HD void lane_body(const uint8_t *src, uint8_t *dst, uint64_t pixels, uint32_t bpp, uint32_t tile, uint32_t tiles, uint32_t lane)
{
    if constexpr (KIND == K_COPY && FORM == F_ALIGNED) {
        // A copy moves bytes, whatever a pixel is: the tile's kWorkgroup * bpp quads of 16 bytes go kWorkgroup at a time, quad
        // k * kWorkgroup + lane in step k, so that every load and store instruction of a wavefront covers consecutive bytes
        // (16 pixels a lane would stride them 16 * bpp apart: measured 1.7 x the time of a plain copy).  The
        // image's last bytes % 16 go byte by byte, in its first workgroup.
        const uint64_t bytes = pixels * bpp, quads = bytes / 16;
        for (uint64_t t = tile; t * kTilePixels < pixels; t += tiles) {
            const uint64_t first = t * (kTilePixels / 16) * bpp + lane;
            Quad q[4]; // (every load before the first store: the stores would order the loads behind them)
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (k < bpp && first + k * kWorkgroup < quads) q[k] = load_quad(src, first + k * kWorkgroup);
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (k < bpp && first + k * kWorkgroup < quads) store_quad(dst, first + k * kWorkgroup, q[k]);
        }
        if (tile == 0 && lane < bytes % 16) dst[quads * 16 + lane] = src[quads * 16 + lane];
        return;
    }
    const uint32_t sb = src_bpp(KIND, bpp), db = dst_bpp(KIND, bpp);
    for (uint64_t t = tile; t * kTilePixels < pixels; t += tiles) {
        const uint64_t first = t * kTilePixels + (uint64_t)lane * kLanePixels;
        if (first >= pixels) return; // (so are this lane's groups of the tiles behind)
        const uint64_t left = pixels - first;
        const uint8_t *s = src + first * sb;
        uint8_t *d = dst + first * db;
        if constexpr (FORM == F_ALIGNED && KIND != K_COPY) {
            if (left >= kLanePixels) {
                constexpr int sw = (int)src_bpp(KIND, 1), dw = (int)dst_bpp(KIND, 1); // dwordx4 in, dwordx4 out
                uint32_t in[4 * sw], out[4 * dw];
#pragma unroll
                for (int k = 0; k < sw; ++k) {
                    const Quad q = load_quad(s, (uint32_t)k);
                    in[4 * k] = q.x; in[4 * k + 1] = q.y; in[4 * k + 2] = q.z; in[4 * k + 3] = q.w;
                }
                convert16<KIND>(in, out);
#pragma unroll
                for (int k = 0; k < dw; ++k) {
                    Quad q;
                    q.x = out[4 * k]; q.y = out[4 * k + 1]; q.z = out[4 * k + 2]; q.w = out[4 * k + 3];
                    store_quad(d, (uint32_t)k, q);
                }
                continue;
            }
        }
        const uint32_t n = left < kLanePixels ? (uint32_t)left : kLanePixels;
        for (uint32_t k = 0; k < n; ++k) convert_pixel<KIND>(s + (uint64_t)k * sb, d + (uint64_t)k * db, bpp);
    }
}

// ---- the ragged launch ----------------------------------------------------------------------------------------------------------
// One image of a launch.  A launch is a flat 1-D grid over all tiles of its images, which are all of one class (kind x form).
struct Record {
    uint64_t src;        // the address of the image's first source byte
    uint64_t dst;        // ... of its first destination byte
    uint64_t pixels;     // width * height
    uint32_t first_tile; // its first tile in the launch: the tiles of the records in front of it summed
    uint32_t tiles;      // its tiles: the workgroups that stride over it
    uint32_t bpp;        // K_COPY: bytes per pixel, 1..4 (the other kinds' are their own)
    uint32_t reserved;
};
static_assert(sizeof(Record) == 40, "uploaded as it is");

// The image that holds tile t of the launch: the last record whose first_tile is not behind t.  count >= 1, first_tile[0] ==
// 0, strictly ascending (every image has a tile).  Table: a pointer to records (the kernels pass one into the constant
// address space: t is uniform across a workgroup, so the loads are scalar ones).
template <class Table> PIXO_CV_HD uint32_t image_of_tile(Table t, uint32_t count, uint32_t tile)
{
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (t[mid].first_tile <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}
// The tiles of an image of `pixels` (>= 1) pixels under a cap of image_tiles (>= 1)
PIXO_CV_HD uint32_t tiles_of(uint64_t pixels, uint32_t image_tiles)
{
    const uint64_t whole = (pixels + kTilePixels - 1) / kTilePixels;
    return (uint32_t)(whole < image_tiles ? whole : image_tiles);
}
// The form of an image from its two addresses
PIXO_CV_HD int form_of(uint64_t src, uint64_t dst) { return ((src | dst) & 15) == 0 ? F_ALIGNED : F_BYTES; }
PIXO_CV_HD uint32_t class_of(int kind, int form) { return (uint32_t)kind * kForms + (uint32_t)form; }

// ---- host: the table of a sub-batch ---------------------------------------------------------------------------------------------
struct Item { // one image of the sub-batch, in index order
    uint64_t src, dst, pixels;
    uint32_t kind, bpp;
};
struct Launch {
    uint32_t cls;                 // class_of(kind, form) of all its images
    uint32_t first_record, count; // its records in the table
    uint32_t tiles;               // their tiles summed: the grid
};
// items (index order) -> the records grouped by class (ascending, index order inside a class) and one Launch per class
// present.  record_item[r]: the item record r describes.  False: the tiles of a launch exceed launch_tiles (the driver ends a
// sub-batch before that).
inline bool build_table(const std::vector<Item> &items, uint32_t image_tiles, uint64_t launch_tiles, std::vector<Record> &table,
                        std::vector<Launch> &launches, std::vector<uint32_t> &record_item)
{
    const uint32_t n = (uint32_t)items.size();
    std::vector<uint32_t> order(n), cls(n);
    for (uint32_t k = 0; k < n; ++k) { order[k] = k; cls[k] = class_of((int)items[k].kind, form_of(items[k].src, items[k].dst)); }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cls[a] < cls[b]; });
    table.clear(); launches.clear(); record_item.clear();
    for (uint32_t r = 0; r < n; ++r) {
        const uint32_t k = order[r];
        const Item &it = items[k];
        if (launches.empty() || launches.back().cls != cls[k]) launches.push_back(Launch{cls[k], r, 0, 0});
        Launch &l = launches.back();
        const uint32_t tiles = tiles_of(it.pixels, image_tiles);
        if ((uint64_t)l.tiles + tiles > launch_tiles) return false;
        table.push_back(Record{it.src, it.dst, it.pixels, l.tiles, tiles, it.bpp, 0});
        record_item.push_back(k);
        l.tiles += tiles;
        l.count += 1;
    }
    return true;
}

} // namespace pixo_convert
