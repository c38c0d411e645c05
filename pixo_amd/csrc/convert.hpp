// convert.hpp — host-callable launchers of the colour-conversion kernels (convert.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "convert_math.h"

namespace pixo_dev {

// One image: `pixels` pixels at d_src -> d_dst, kind and form as convert_math.h (form from the two addresses: form_of), over
// `tiles` workgroups (tiles_of).  bpp: K_COPY's bytes per pixel.
hipError_t launch_convert(const uint8_t *d_src, uint8_t *d_dst, uint64_t pixels, uint32_t bpp, int kind, int form, uint32_t tiles, hipStream_t stream);
// One flat launch over the `tiles` tiles of `count` records of one class (device memory, as build_table made them)
hipError_t launch_convert_images(const pixo_convert::Record *d_records, uint32_t count, uint32_t tiles, int kind, int form, hipStream_t stream);

} // namespace pixo_dev
