// resize.hpp — host-callable launchers of the resize kernels (resize.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "resize_images_math.h"

namespace pixo_dev {

// One axis of a Lanczos3 contribution table as the kernels read it (device pointers): the taps of destination index d are
// source indices start[d] .. start[d] + (off[d + 1] - off[d]), their weights w[off[d]] ...
struct ResizeAxisTable {
    const uint32_t *start;
    const uint32_t *off; // dst + 1 entries
    const float *w;
};

// The intermediate's rows are padded to this many bytes so that the vertical pass loads aligned dwords
inline size_t resize_mid_stride(uint32_t dst_w, uint32_t bpp) { return (static_cast<size_t>(dst_w) * bpp + 15) & ~size_t{15}; }

// Nearest (algorithm 0) or bilinear (1): d_src [sh][sw][bpp] -> d_dst [dh][dw][bpp]
hipError_t launch_resize_point(const uint8_t *d_src, uint32_t sw, uint32_t sh, uint8_t *d_dst, uint32_t dw, uint32_t dh, uint32_t bpp,
                               int algorithm, hipStream_t stream);
// Lanczos3, horizontal pass: d_src [sh][sw][bpp] -> d_mid, sh rows of resize_mid_stride(dw, bpp) bytes.  max_span: the
// largest number of source pixels the outputs of one workgroup (kResizeHTile adjacent destination columns) cover; spans
// that fit the kernel's LDS segment are staged there, longer ones are read from memory directly.
constexpr uint32_t kResizeHTile = 64;
hipError_t launch_resize_lanczos_h(const uint8_t *d_src, uint32_t sw, uint32_t sh, uint8_t *d_mid, uint32_t dw, uint32_t bpp,
                                   ResizeAxisTable t, uint32_t max_span, hipStream_t stream);
// ... vertical pass: d_mid -> d_dst [dh][dw][bpp]
hipError_t launch_resize_lanczos_v(const uint8_t *d_mid, uint32_t sh, uint8_t *d_dst, uint32_t dw, uint32_t dh, uint32_t bpp,
                                   ResizeAxisTable t, hipStream_t stream);
// The horizontal kernel's LDS segment per source row, and whether a tile of `max_span` source pixels is staged in it: the
// staged segment keeps the source's alignment (up to 3 bytes in front) and is stored in whole dwords
constexpr uint32_t kResizeSegBytes = 8192;
inline bool resize_h_uses_lds(uint32_t max_span, uint32_t bpp) { return static_cast<size_t>(max_span) * bpp + 8 <= size_t{kResizeSegBytes}; }

// ---- batches: n sources of individual sizes -> n images of one destination size, back to back at d_dst ---------------------
// What a workgroup of a batch kernel reads about its image (blockIdx.z).  The tables of all axes lie in one block: an axis
// with destination size n at byte offset `at` (a multiple of 16) is start[n], off[n + 1], w[...] as in ResizeAxisTable.
struct ResizeBatchItem {
    const uint8_t *src;  // [sh][sw][bpp]
    uint64_t mid_at;     // Lanczos3: where the image's sh rows of the intermediate start (bytes, a multiple of 16)
    uint64_t h_at, v_at; // ... its horizontal (sw -> dw) and vertical (sh -> dh) axis in the block of tables
    uint32_t sw, sh;
    uint32_t use_lds;    // ... the horizontal pass stages this image's tiles in LDS
    uint32_t reserved;
};
static_assert(sizeof(ResizeBatchItem) == 48, "uploaded as it is");
// grid.z = n <= 65535 images; d_items and d_tables are device memory.  Image i is written at d_dst + i * dw * dh * bpp.
hipError_t launch_resize_point_batch(const ResizeBatchItem *d_items, uint32_t n, uint8_t *d_dst, uint32_t dw, uint32_t dh, uint32_t bpp,
                                     int algorithm, hipStream_t stream);
// max_sh: the tallest source among the n (sizes grid.y; workgroups beyond a shorter image's rows leave at once)
hipError_t launch_resize_lanczos_h_batch(const ResizeBatchItem *d_items, uint32_t n, uint32_t max_sh, const uint8_t *d_tables, uint8_t *d_mid,
                                         uint32_t dw, uint32_t bpp, hipStream_t stream);
hipError_t launch_resize_lanczos_v_batch(const ResizeBatchItem *d_items, uint32_t n, const uint8_t *d_tables, const uint8_t *d_mid, uint8_t *d_dst,
                                         uint32_t dw, uint32_t dh, uint32_t bpp, hipStream_t stream);

// ---- images: n sources of individual sizes -> n images of individual sizes, anywhere (resize_images_math.h) ----------------
// One flat launch over the `tiles` tiles of `count` records (device memory, as build_table made them for the pass); every image
// of a point or horizontal launch has `bpp` bytes a pixel, the vertical launch takes images of any.  d_tables: the block of
// axis tables h_at / v_at count from; d_mid: the sub-batch's intermediate mid_at counts from.
hipError_t launch_resize_point_images(const pixo_resize_images::Record *d_records, uint32_t count, uint32_t tiles, uint32_t bpp, int algorithm,
                                      hipStream_t stream);
hipError_t launch_resize_lanczos_h_images(const pixo_resize_images::Record *d_records, uint32_t count, uint32_t tiles, const uint8_t *d_tables,
                                          uint8_t *d_mid, uint32_t bpp, hipStream_t stream);
hipError_t launch_resize_lanczos_v_images(const pixo_resize_images::Record *d_records, uint32_t count, uint32_t tiles, const uint8_t *d_tables,
                                          const uint8_t *d_mid, hipStream_t stream);

} // namespace pixo_dev
