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

} // namespace pixo_dev
