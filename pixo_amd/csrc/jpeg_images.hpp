// jpeg_images.hpp — host-callable launcher of the ragged coefficient kernel (jpeg_images.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "jpeg_images_math.h"

namespace pixo_dev {

// Enqueues the colour -> DCT -> quantise kernel over the `tiles` tiles of `count` images of ONE class — mode
// (pixo_jpeg_images::MODE_*) and load form (LOAD_*) — described by d_records (device memory, uploaded before the launch).
// Every image's planes land at its record's block offsets from d_tuple; d_qt: the table block of the requested quality.
hipError_t launch_jpeg_images_coeffs(int mode, int load, const pixo_jpeg_images::TileRecord *d_records, uint32_t count, uint32_t tiles,
                                     int16_t *d_tuple, const float *d_qt, hipStream_t stream);

} // namespace pixo_dev
