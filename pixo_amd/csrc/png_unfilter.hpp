// png_unfilter.hpp — launchers of the PNG decoder's device stage (png_unfilter.hip): row reconstruction on the skewed
// wavefront, then the conversion to 8-bit pixels.  The arithmetic is png_unfilter_math.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "png_unfilter_math.h"

namespace pixo_dev {

// Rows a workgroup reconstructs side by side (a row per lane of its one wavefront); a longer run of rows is walked in
// passes of this many.
constexpr uint32_t kUnfilterPassRows = 64;
// Bytes a lane reads and writes at a time, and by which it lags the lane above.
constexpr uint32_t kUnfilterPiece = 16;

inline uint64_t unfilter_pitch(uint64_t row_bytes) { return (row_bytes + kUnfilterPiece - 1) / kUnfilterPiece * kUnfilterPiece; }
// Bytes the stream's buffer must hold: a lane's last piece may read up to 15 bytes past the end of the last row.
inline uint64_t unfilter_stream_alloc(uint64_t height, uint64_t row_bytes) { return height * (row_bytes + 1) + kUnfilterPiece; }

struct UnfilterArgs {
    const uint8_t *stream;  // height rows of 1 filter byte (0..4, checked by the caller) + row_bytes bytes; unfilter_stream_alloc bytes
    uint8_t *rows;          // out: the reconstructed rows, `pitch` bytes apart (16-byte aligned, height * pitch bytes)
    uint64_t row_bytes, pitch;
    uint32_t bpp;           // the filter unit: 1, 2, 3, 4, 6 or 8
    const uint32_t *runs;   // n_runs pairs (first row, rows): every run starts at a row that does not read the row above
    uint32_t n_runs;        //   (row 0, or filter None / Sub) and the runs cover rows 0 .. height - 1 exactly once
};
hipError_t launch_png_unfilter(const UnfilterArgs &a, hipStream_t stream);

struct UnconvertArgs {
    const uint8_t *rows;    // the reconstructed rows
    uint64_t pitch;
    uint8_t *out;           // width * height * out_bpp bytes
    uint32_t width, height;
    uint32_t form;          // pixo_pngu::Convert
    uint32_t depth;         // bits per sample in the rows
    uint32_t out_bpp;       // bytes per output pixel
    const uint32_t *table;  // CONVERT_PALETTE: 256 words r | g << 8 | b << 16 | a << 24
};
hipError_t launch_png_convert(const UnconvertArgs &a, hipStream_t stream);

// ---- batches: the runs of many images in one unfilter launch per filter unit, their conversion in one launch per kernel form ----
// One image of a batch, as both kernels read it (wavefront-uniform: a workgroup serves one image).
struct UnfilterBatchImage {
    uint64_t stream_at;     // its stream's offset in the sub-batch's stream buffer
    uint64_t rows_at;       // its reconstructed rows' offset in the sub-batch's rows buffer (a multiple of 16)
    uint64_t row_bytes, pitch;
    uint64_t out_at;        // its pixels' offset from d_pixels
    uint32_t width, height;
    uint32_t form, depth, out_bpp; // as UnconvertArgs
    uint32_t aligned4;      // d_pixels + out_at is a multiple of 4: dword stores
    uint32_t table_at;      // CONVERT_PALETTE: its 256 words' offset, in words, in the batch's palette tables
    uint32_t reserved[3];
}; // 80 bytes
static_assert(sizeof(UnfilterBatchImage) == 80, "a multiple of 16: the descriptions lie back to back");
// One run of rows: a workgroup of the batch unfilter kernel
struct UnfilterBatchRun {
    uint32_t image, first_row, rows, reserved;
};
static_assert(sizeof(UnfilterBatchRun) == 16, "read as one 16-byte word");

// The kernel forms of the conversion: which one serves an image is the caller's choice, by launch_png_convert's rule applied
// to the REAL address d_pixels + out_at.
enum ConvertKernel : uint32_t { CONVERT_KERNEL_COPY16 = 0, CONVERT_KERNEL_BYTES = 1, CONVERT_KERNEL_SAMPLES = 2, CONVERT_KERNELS = 3 };
inline uint32_t convert_kernel_of(uint32_t form, uint64_t row_out, uintptr_t out)
{
    if (form == pixo_pngu::CONVERT_COPY || form == pixo_pngu::CONVERT_HIGH)
        return form == pixo_pngu::CONVERT_COPY && row_out % 16 == 0 && out % 16 == 0 ? CONVERT_KERNEL_COPY16 : CONVERT_KERNEL_BYTES;
    return CONVERT_KERNEL_SAMPLES;
}

struct UnfilterBatchArgs {
    const uint8_t *stream;            // the sub-batch's streams; the buffer ends at least 16 bytes behind the last stream
    uint8_t *rows;                    // out: the sub-batch's reconstructed rows (16-byte aligned)
    const UnfilterBatchImage *images; // the batch's descriptions
    const UnfilterBatchRun *runs;     // n_runs runs of images whose filter unit is `bpp` (per image: as UnfilterArgs::runs)
    uint32_t n_runs, bpp;
};
hipError_t launch_png_unfilter_batch(const UnfilterBatchArgs &a, hipStream_t stream);

struct UnconvertBatchArgs {
    const uint8_t *rows;              // the sub-batch's reconstructed rows
    uint8_t *out;                     // d_pixels (any alignment)
    const UnfilterBatchImage *images;
    const uint32_t *list;             // the launch's block table: blockIdx.y -> image, n entries, all of kernel form `kernel`
    uint32_t n, kernel;
    const uint32_t *tables;           // the batch's palette tables
    uint64_t max_items;               // the most work items (16-byte pieces, dwords, pixels) any image of the list has
};
hipError_t launch_png_convert_batch(const UnconvertBatchArgs &a, hipStream_t stream);

} // namespace pixo_dev
