// convert.hip — colour conversion on the device: GrayAlpha -> Gray, Rgba -> Rgb, Rgb / Rgba -> Gray (the reference front
// end's gray_alpha_to_gray, rgba_to_rgb and to_grayscale, src/bin/pixo.rs:478-513) and the plain copy of an image that keeps
// its type.  Element-wise and memory-bound: a workgroup of 256 lanes takes a tile of 4096 consecutive pixels, a lane 16 of
// them — in the aligned form as whole dwordx4 loads and stores (64 -> 48, 32 -> 16, 48 -> 16, 64 -> 16 bytes), in the byte
// form pixel by pixel.  The body is convert_math.h's lane_body, the same code the host emulation runs.  Two kernels per
// (kind, form): one image by its arguments, and the ragged launch that finds its image by a scalar search over a table.
#include <hip/hip_runtime.h>

#include "convert.hpp"

namespace {

namespace cv = pixo_convert;
static_assert(cv::kTilePixels == 256 * 16 && cv::kWorkgroup == 256, "a tile is what a workgroup's lanes take in one step");
// The table of a ragged launch was uploaded before the launch and nothing writes it: read through the constant address
// space, the search (its tile index is blockIdx.x) and the record are scalar loads, the values stay in scalar registers.
using ConstRecord = const __attribute__((address_space(4))) cv::Record;

template <int KIND, int FORM>
__global__ __launch_bounds__(256) void convert_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t pixels, uint32_t bpp,
                                                      uint32_t tiles)
{
    cv::lane_body<KIND, FORM>(src, dst, pixels, bpp, blockIdx.x, tiles, threadIdx.x);
}

template <int KIND, int FORM> __global__ __launch_bounds__(256) void convert_images_kernel(const cv::Record *__restrict__ records, uint32_t count)
{
    ConstRecord *table = (ConstRecord *)records;
    ConstRecord *im = table + cv::image_of_tile(table, count, blockIdx.x);
    cv::lane_body<KIND, FORM>(reinterpret_cast<const uint8_t *>(im->src), reinterpret_cast<uint8_t *>(im->dst), im->pixels, im->bpp,
                              blockIdx.x - im->first_tile, im->tiles, threadIdx.x);
}

} // namespace

namespace pixo_dev {

#define PIXO_CV_KIND(K)                                      \
    case K:                                                  \
        if (form == cv::F_ALIGNED) PIXO_CV_GO(K, cv::F_ALIGNED); \
        else PIXO_CV_GO(K, cv::F_BYTES);                     \
        break
#define PIXO_CV_KINDS()                                                                                                     \
    switch (kind) {                                                                                                         \
        PIXO_CV_KIND(cv::K_COPY); PIXO_CV_KIND(cv::K_GA_G); PIXO_CV_KIND(cv::K_RGBA_RGB); PIXO_CV_KIND(cv::K_RGB_G); PIXO_CV_KIND(cv::K_RGBA_G); \
    default: return hipErrorInvalidValue;                                                                                   \
    }

hipError_t launch_convert(const uint8_t *d_src, uint8_t *d_dst, uint64_t pixels, uint32_t bpp, int kind, int form, uint32_t tiles, hipStream_t stream)
{
    if (tiles == 0 || tiles > cv::kMaxTiles) return hipErrorInvalidValue;
#define PIXO_CV_GO(K, F) hipLaunchKernelGGL((convert_kernel<K, F>), dim3(tiles), dim3(256), 0, stream, d_src, d_dst, pixels, bpp, tiles)
    PIXO_CV_KINDS()
#undef PIXO_CV_GO
    return hipGetLastError();
}

hipError_t launch_convert_images(const cv::Record *d_records, uint32_t count, uint32_t tiles, int kind, int form, hipStream_t stream)
{
    if (count == 0 || tiles == 0 || tiles > cv::kMaxTiles) return hipErrorInvalidValue;
#define PIXO_CV_GO(K, F) hipLaunchKernelGGL((convert_images_kernel<K, F>), dim3(tiles), dim3(256), 0, stream, d_records, count)
    PIXO_CV_KINDS()
#undef PIXO_CV_GO
    return hipGetLastError();
}

} // namespace pixo_dev
