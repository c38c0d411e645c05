// png_inflate_dev.hpp — launchers of the device inflate of the PNG decode batches (png_inflate.hip): N zlib streams in
// device memory -> N inflated streams, a workgroup of one wavefront per stream; then the filter bytes of every image gathered
// into one compact array.  The arithmetic is png_inflate_math.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "png_inflate_math.h"

namespace pixo_dev {

// Where a stream's input must start (a multiple of this) and how many readable zero bytes must follow it
constexpr uint32_t kInflateInputAlign = 16;

// One stream, as its workgroup reads it (wavefront-uniform)
struct InflateStream {
    uint64_t in_at;     // its DEFLATE bytes — the zlib stream without its 2-byte header and its 4-byte checksum — in `input`: a
    uint64_t in_len;    //   multiple of 16, followed by at least 16 zero bytes
    uint64_t out_at;    // [out_at, out_at + expected) of `out` is all the kernel writes for it
    uint64_t expected;
};
static_assert(sizeof(InflateStream) == 32, "the descriptions lie back to back");
// What its workgroup leaves: `produced` bytes of the region are inflated bytes whose Adler-32 is `adler`, whatever the verdict
struct InflateStatus {
    uint32_t verdict; // pixo_pngi::Verdict
    uint32_t adler;
    uint64_t produced;
};
static_assert(sizeof(InflateStatus) == 16, "one 16-byte record per stream");

struct InflateArgs {
    const uint8_t *input;         // 16-byte aligned
    uint8_t *out;
    const InflateStream *streams; // n of them
    InflateStatus *status;        // n records
    uint32_t n;
};
hipError_t launch_png_inflate(const InflateArgs &a, hipStream_t stream);

// One image's filter bytes: byte y of its `height` bytes at filters + filters_at is stream[stream_at + y * stride]
struct FilterGatherImage {
    uint64_t stream_at, stride, filters_at;
    uint32_t height, reserved;
};
static_assert(sizeof(FilterGatherImage) == 32, "the descriptions lie back to back");
struct FilterGatherArgs {
    const uint8_t *stream;
    uint8_t *filters;
    const FilterGatherImage *images; // n of them
    uint32_t n, max_height;
};
hipError_t launch_png_filter_gather(const FilterGatherArgs &a, hipStream_t stream);

} // namespace pixo_dev
