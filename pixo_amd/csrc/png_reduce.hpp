// png_reduce.hpp — host-callable launchers of the PNG reduction kernels (png_reduce.hip): what the reference does to the
// pixels between its caller and apply_filters (src/png/mod.rs:522-554).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "png_reduce_math.h"

namespace pixo_dev {

// What one read pass learns about an image.  A flag is set as soon as one pixel proves it; a pass that has
// proven everything it was asked about leaves early.
enum : uint32_t {
    PNG_A_OVERFLOW = 1,   // more than 256 distinct colour keys
    PNG_A_NON_OPAQUE = 2, // a pixel with alpha != 255
    PNG_A_NON_GRAY = 4,   // a pixel with r != g or g != b
    PNG_A_ALPHA0 = 8,     // a pixel with alpha == 0
};
struct PngAnalysis {
    uint32_t flags;    // PNG_A_*
    uint32_t gray_max; // maximum of the first channel (meaningful when no pixel set PNG_A_NON_GRAY)
    uint32_t count;    // distinct colour keys in `table` (meaningful without PNG_A_OVERFLOW)
    uint32_t pad;
    uint64_t table[pixo_pngr::kSetSlots]; // the keys: used slots carry pixo_pngr::kSlotUsed
};

// `want`: the PNG_A_* questions to answer (PNG_A_OVERFLOW: build the colour set).  spp: 2 (alpha only), 3 or 4.
// d_state is zeroed on the stream first.
hipError_t launch_png_analyse(const void *d_pixels, uint64_t pixels, uint32_t spp, uint32_t want, PngAnalysis *d_state,
                              hipStream_t stream);
// Pixels -> index into the sorted keys (d_lookup: kSetSlots slots with the index in bits 32-39) and the histogram of
// the indices (d_hist: 256 u32, zeroed on the stream first).  d_index holds `pixels` bytes rounded up to 4.
hipError_t launch_png_index(const void *d_pixels, uint64_t pixels, uint32_t spp, const uint64_t *d_lookup, uint8_t *d_index,
                            uint32_t *d_hist, hipStream_t stream);
// d_pairs[a * n + b], a < b: how many horizontally or vertically adjacent pixel pairs have the indices {a, b}
// (n * n u32, zeroed on the stream first; pairs of equal indices are not counted: nothing reads the diagonal).
hipError_t launch_png_cooccurrence(const uint8_t *d_index, uint32_t width, uint32_t height, uint32_t n, uint32_t *d_pairs,
                                   hipStream_t stream);
// The reduced rows: height * row_bytes bytes, tightly packed, into d_dst (capacity rounded up to 4 bytes).
hipError_t launch_png_convert(const pixo_pngr::ConvertArgs &a, const void *d_src, const uint8_t *d_map, void *d_dst,
                              hipStream_t stream);

} // namespace pixo_dev
