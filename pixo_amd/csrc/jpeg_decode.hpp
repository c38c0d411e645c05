// jpeg_decode.hpp — host-callable launcher of the JPEG decode kernel (jpeg_decode.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "jpeg_decode_math.h"

namespace pixo_dev {

// One flat launch over the `tiles` tiles of `count` records of one class and form (device memory, in launch order): d_coef the
// sub-batch's coefficients, d_pixels the address the records' out_at count from.
hipError_t launch_jpeg_decode(const pixo_jdec::Record *d_records, uint32_t count, uint32_t tiles, int cls, int form, const uint8_t *d_coef,
                              uint8_t *d_pixels, hipStream_t stream);

} // namespace pixo_dev
