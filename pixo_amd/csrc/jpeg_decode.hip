// jpeg_decode.hip — baseline JPEG decode behind the host's entropy decoder: quantised coefficients in HBM -> pixels in HBM.  One
// launch per class of images (gray, 4:4:4, 4:2:2, 4:2:0; each with 16-byte stores or byte stores) over the tiles of all the
// class's images: a workgroup finds its image by a scalar search over the launch's records, owns a tile of 16 x 4 whole MCUs,
// and runs jpeg_decode_math.h's two phases around one barrier.  Phase A: a lane per 8x8 block — eight dwordx4 loads, dequantise,
// both IDCT passes in registers, samples to the tile's planes in LDS; the chroma planes of a subsampled class carry a ring of
// blocks around the tile's own (the halo), transformed again here, because the upsampler reads one sample beyond the tile.
// Phase B: fancy upsampling, colour conversion and the crop, stored in runs of 16 pixels.  The bytes between two images and
// behind an image's end are never written.
#include <hip/hip_runtime.h>

#include "jpeg_decode.hpp"

namespace {

namespace jd = pixo_jdec;
// The records were uploaded before the launch and nothing writes them: read through the constant address space, the search
// (its tile index is blockIdx.x) and the record's fields are scalar loads.
using ConstRecord = const __attribute__((address_space(4))) jd::Record;

template <int CLS, int FORM>
__global__ __launch_bounds__(256) void jpeg_decode_kernel(const jd::Record *__restrict__ records, uint32_t count, const uint8_t *__restrict__ coef,
                                                          uint8_t *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint8_t planes[jd::lds_bytes(CLS)];
    ConstRecord *table = (ConstRecord *)records;
    ConstRecord *im = table + jd::image_of_tile(table, count, blockIdx.x);
    const uint32_t tile = blockIdx.x - im->first_tile;
    jd::phase_a<CLS>(im, coef, planes, tile, threadIdx.x, jd::kWorkgroup);
    __syncthreads();
    jd::phase_b<CLS, FORM>(im, planes, out + im->out_at, tile, threadIdx.x, jd::kWorkgroup);
}

} // namespace

namespace pixo_dev {

hipError_t launch_jpeg_decode(const pixo_jdec::Record *d_records, uint32_t count, uint32_t tiles, int cls, int form, const uint8_t *d_coef,
                              uint8_t *d_pixels, hipStream_t stream)
{
    if (count == 0 || tiles == 0 || tiles > jd::kMaxTiles) return hipErrorInvalidValue;
#define PIXO_JD_GO(C, F) hipLaunchKernelGGL((jpeg_decode_kernel<C, F>), dim3(tiles), dim3(jd::kWorkgroup), 0, stream, d_records, count, d_coef, d_pixels)
#define PIXO_JD_CLASS(C)                                          \
    case C:                                                       \
        if (form == jd::F_ALIGNED) PIXO_JD_GO(C, jd::F_ALIGNED);  \
        else PIXO_JD_GO(C, jd::F_BYTES);                          \
        break
    switch (cls) {
        PIXO_JD_CLASS(jd::C_GRAY); PIXO_JD_CLASS(jd::C_444); PIXO_JD_CLASS(jd::C_422); PIXO_JD_CLASS(jd::C_420);
    default: return hipErrorInvalidValue;
    }
#undef PIXO_JD_CLASS
#undef PIXO_JD_GO
    return hipGetLastError();
}

} // namespace pixo_dev
