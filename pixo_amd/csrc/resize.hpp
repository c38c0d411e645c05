// resize.hpp — host-callable launchers of the resize kernels (resize.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

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

} // namespace pixo_dev
