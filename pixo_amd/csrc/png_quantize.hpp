// png_quantize.hpp — host-callable launchers of the PNG quantisation kernels (png_quantize.hip): the device side of
// quantize_image (src/png/mod.rs:1505-1701).  Palettes travel as colour keys (r<<24 | g<<16 | b<<8 | a).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "png_quantize_math.h"

namespace pixo_dev {

// d_keys[i] = key of pixel i * stride_a for i < count_a, then of pixel (i - count_a) * stride_b for count_b more.
hipError_t launch_pngq_gather(const void *d_pixels, uint32_t spp, uint64_t stride_a, uint32_t count_a, uint64_t stride_b, uint32_t count_b,
                              uint32_t *d_keys, hipStream_t stream);
// One k-means assignment round: every colour goes to its nearest palette entry (first minimum); d_acc[5 * i + 0..4] receive
// the count-weighted sums of r, g, b, a and the count of entry i (u64; zeroed on the stream first).
hipError_t launch_pngq_assign(const uint32_t *d_colors, const uint32_t *d_counts, uint32_t n_colors, const uint32_t *d_palette, uint32_t n,
                              unsigned long long *d_acc, hipStream_t stream);
// The 64^3 cells' nearest entries: d_lut holds kLutCells bytes (4-byte aligned).
hipError_t launch_pngq_lut(const uint32_t *d_palette, uint32_t n, uint8_t *d_lut, hipStream_t stream);
// Pixels -> indices without dithering.  d_lut null: the search for every pixel (the early out's exact lookup, :1583-1614).
hipError_t launch_pngq_map(const void *d_pixels, uint64_t pixels, uint32_t spp, const uint8_t *d_lut, const uint32_t *d_palette, uint32_t n,
                           uint8_t *d_index, hipStream_t stream);

// Floyd-Steinberg.  bands = ceil(height / kBandRows).  d_carry: width u64 per band (what the band above leaves for a band's
// first row); d_state: kDitherStateWords u32 ([0] ticket, [1] a band gave up).  chained: one launch of `bands` workgroups
// that take their band from the ticket and wait — at most spin_budget polls per column — for the band above, column by column;
// both buffers are zeroed on the stream first.  Not chained: band `only_band` alone, the bands above it complete (launches in
// stream order); nothing waits.
constexpr uint32_t kDitherStateWords = 4;
struct DitherArgs {
    const uint8_t *px;
    uint32_t spp, width, height;
    const uint8_t *lut;
    const uint32_t *palette;
    uint32_t n;
    uint8_t *index;
    unsigned long long *carry;
    uint32_t *state;
};
hipError_t launch_pngq_dither_chained(const DitherArgs &a, uint32_t spin_budget, hipStream_t stream);
hipError_t launch_pngq_dither_band(const DitherArgs &a, uint32_t only_band, hipStream_t stream);

} // namespace pixo_dev
