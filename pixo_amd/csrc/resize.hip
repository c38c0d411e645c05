// resize.hip — pixo::resize on the device (reference src/resize.rs): nearest and bilinear in one kernel, Lanczos3 as the
// reference's two separable passes with its u8 intermediate between them.  The arithmetic is resize_math.h's, shared with
// the host; this file is the memory side.  All three are byte-gather kernels with 1-4 bytes per pixel.
//
//   resize_point_kernel      a thread owns four adjacent output pixels of a row; the column terms (x0 / x1 / frac, or the
//                            nearest column) are computed once per thread and serve every channel and every row the
//                            thread visits.  The 4 * bpp output bytes leave as bpp dwords where the address allows.
//   resize_lanczos_h_kernel  a wavefront owns 64 adjacent output columns of one source row, a workgroup four such rows.  The
//                            source bytes those 64 outputs cover (neighbours share most taps) are staged in LDS by aligned
//                            dword loads; each lane then walks its taps in order, one accumulator per channel.
//   resize_lanczos_v_kernel  a thread owns four adjacent BYTES of an output row (the vertical pass treats every byte column
//                            alike, whatever the pixel size): per tap the workgroup reads consecutive aligned dwords of one
//                            intermediate row (rows padded to 16 bytes), the tap's weight is uniform over the workgroup.
//
// Each of the three is a __device__ body, which takes its tile's coordinates and the row stride as parameters, with three
// __global__ entries: the single one (one image, its shape in the kernel arguments; the tile is blockIdx.x / .y), the batch
// one (blockIdx.z is the image: every workgroup reads its image's ResizeBatchItem, then walks the same body: N sources of
// individual sizes to N images of ONE destination size, written back to back) and the images one (a flat 1-D grid over
// the tiles of images of individual source AND destination sizes: every workgroup finds its image's Record by a binary
// search with its uniform tile index — resize_images_math.h — then walks the same body).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "resize.hpp"
#include "resize_images_math.h"
#include "resize_math.h"

namespace {

constexpr int kSegBytes = pixo_dev::kResizeSegBytes; // LDS bytes per staged source row segment (four rows per workgroup: 32 KiB)

namespace rzi = pixo_resize_images;
static_assert(rzi::kPointTileCols == 64 * 4 && rzi::kPointTileRows == 4 && rzi::kHTileCols == pixo_dev::kResizeHTile && rzi::kHTileRows == 4 &&
                  rzi::kVTileBytes == 256 * 4 && rzi::kVTileRows == 1,
              "the tiles the table counts are the workgroups' of the bodies below");
// The table of a ragged launch was uploaded before the launch and nothing writes it: read through the constant address
// space, the search (its tile index is blockIdx.x) and the record are scalar loads, the values stay in scalar registers.
using ConstRecord = const __attribute__((address_space(4))) rzi::Record;
struct TileOf {
    ConstRecord *im;
    uint32_t tx, ty;
};
__device__ __forceinline__ TileOf tile_of(const rzi::Record *records, uint32_t count)
{
    ConstRecord *table = (ConstRecord *)records;
    TileOf t;
    t.im = table + rzi::image_of_tile(table, count, blockIdx.x);
    rzi::tile_in_image(blockIdx.x, t.im->first_tile, t.im->tiles_x, &t.tx, &t.ty);
    return t;
}

// ---- nearest / bilinear -----------------------------------------------------------------------------------------------------
template <int BPP> __device__ __forceinline__ void store_group(uint8_t *p, const uint8_t (&o)[4 * BPP], uint32_t pixels)
{
    if (pixels == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < BPP; ++k)
            reinterpret_cast<uint32_t *>(p)[k] = (uint32_t)o[4 * k] | ((uint32_t)o[4 * k + 1] << 8) | ((uint32_t)o[4 * k + 2] << 16) | ((uint32_t)o[4 * k + 3] << 24);
        return;
    }
    for (uint32_t k = 0; k < pixels * BPP; ++k) p[k] = o[k];
}

template <int BPP, int ALGO>
__device__ __forceinline__ void resize_point_body(const uint8_t *__restrict__ src, uint32_t sw, uint32_t sh, uint8_t *__restrict__ dst, uint32_t dw,
                                                  uint32_t dh, size_t tile_x, size_t tile_y, size_t tiles_y)
{
    const size_t gx = tile_x * 64 + threadIdx.x;
    if (gx * 4 >= dw) return;
    const uint32_t x_first = (uint32_t)(gx * 4);
    const uint32_t pixels = dw - x_first < 4 ? dw - x_first : 4;
    uint32_t x0[4], x1[4];
    float fx[4];
    const float xr = ALGO == RZ_NEAREST ? rz_nearest_ratio(sw, dw) : rz_bilinear_ratio(sw, dw);
    const float yr = ALGO == RZ_NEAREST ? rz_nearest_ratio(sh, dh) : rz_bilinear_ratio(sh, dh);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t x = x_first + k < dw ? x_first + k : dw - 1; // (a ragged group repeats the last column; not stored)
        if (ALGO == RZ_NEAREST) { x0[k] = rz_nearest_index(x, xr, sw); x1[k] = x0[k]; fx[k] = 0.0f; }
        else rz_bilinear_axis(x, xr, sw, &x0[k], &x1[k], &fx[k]);
    }
    for (size_t y = tile_y * 4 + threadIdx.y; y < dh; y += tiles_y * 4) {
        uint8_t o[4 * BPP];
        if (ALGO == RZ_NEAREST) {
            const uint8_t *row = src + (size_t)rz_nearest_index((uint32_t)y, yr, sh) * sw * BPP;
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < BPP; ++c) o[k * BPP + c] = row[(size_t)x0[k] * BPP + c];
        } else {
            uint32_t y0, y1;
            float fy;
            rz_bilinear_axis((uint32_t)y, yr, sh, &y0, &y1, &fy);
            const uint8_t *r0 = src + (size_t)y0 * sw * BPP, *r1 = src + (size_t)y1 * sw * BPP;
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < BPP; ++c)
                    o[k * BPP + c] = rz_bilinear_px(r0[(size_t)x0[k] * BPP + c], r0[(size_t)x1[k] * BPP + c], r1[(size_t)x0[k] * BPP + c],
                                                    r1[(size_t)x1[k] * BPP + c], fx[k], fy);
        }
        store_group<BPP>(dst + (y * dw + x_first) * BPP, o, pixels);
    }
}
template <int BPP, int ALGO>
__global__ __launch_bounds__(256) void resize_point_kernel(const uint8_t *__restrict__ src, uint32_t sw, uint32_t sh, uint8_t *__restrict__ dst,
                                                           uint32_t dw, uint32_t dh)
{
    resize_point_body<BPP, ALGO>(src, sw, sh, dst, dw, dh, blockIdx.x, blockIdx.y, gridDim.y);
}
// Image blockIdx.z of a batch: its own source and column terms, its place in the block of outputs.  (An image of 4 * k + 1 .. 3
// bytes puts the next one off a dword: store_group looks at the address.)
template <int BPP, int ALGO>
__global__ __launch_bounds__(256) void resize_point_batch_kernel(const pixo_dev::ResizeBatchItem *__restrict__ items, uint8_t *__restrict__ dst,
                                                                 uint32_t dw, uint32_t dh)
{
    const pixo_dev::ResizeBatchItem it = items[blockIdx.z];
    resize_point_body<BPP, ALGO>(it.src, it.sw, it.sh, dst + (size_t)blockIdx.z * dw * dh * BPP, dw, dh, blockIdx.x, blockIdx.y, gridDim.y);
}
// Tile blockIdx.x of a ragged launch: 256 columns x 4 rows of its image's destination; all images of the launch have BPP
// bytes a pixel.  The image's rows of tiles are capped: the body's row loop strides over the rest.
template <int BPP, int ALGO>
__global__ __launch_bounds__(256) void resize_point_images_kernel(const rzi::Record *__restrict__ records, uint32_t count)
{
    const TileOf t = tile_of(records, count);
    resize_point_body<BPP, ALGO>(reinterpret_cast<const uint8_t *>(t.im->src), t.im->sw, t.im->sh, reinterpret_cast<uint8_t *>(t.im->dst), t.im->dw,
                                 t.im->dh, t.tx, t.ty, t.im->tiles_y);
}

// ---- Lanczos3, horizontal ------------------------------------------------------------------------------------------------------
// Stages bytes [first, first + n) of the image into seg, keeping their alignment: seg[shift + i] = img[first + i] with
// shift = (address of img[first]) % 4.  Whole dwords inside the image are loaded as dwords; the ragged ends byte by byte, so
// that nothing outside [img, img + img_bytes) is touched.  One wavefront (64 lanes) per call.
__device__ __forceinline__ uint32_t stage_segment(const uint8_t *img, size_t img_bytes, size_t first, size_t n, uint8_t *seg, uint32_t lane)
{
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(img + first) & 3);
    const ptrdiff_t word0 = (ptrdiff_t)first - (ptrdiff_t)shift; // index into img of the first staged byte (down to -3)
    const size_t words = (shift + n + 3) / 4;
    for (size_t k = lane; k < words; k += 64) {
        const ptrdiff_t at = word0 + (ptrdiff_t)(4 * k);
        uint32_t v = 0;
        if (at >= 0 && (size_t)at + 4 <= img_bytes) {
            v = *reinterpret_cast<const uint32_t *>(img + at);
        } else {
            for (int j = 0; j < 4; ++j)
                if (at + j >= 0 && (size_t)(at + j) < img_bytes) v |= (uint32_t)img[at + j] << (8 * j);
        }
        reinterpret_cast<uint32_t *>(seg)[k] = v;
    }
    return shift;
}

template <int BPP>
__device__ __forceinline__ void resize_lanczos_h_body(const uint8_t *__restrict__ src, uint32_t sw, uint32_t sh, uint8_t *__restrict__ mid,
                                                      size_t mid_stride, uint32_t dw, pixo_dev::ResizeAxisTable t, int use_lds, size_t tile_x,
                                                      size_t tile_y, size_t tiles_y)
{
    __shared__ __attribute__((aligned(16))) uint8_t seg[4][kSegBytes];
    const size_t d = tile_x * 64 + threadIdx.x;
    const bool col = d < dw;
    uint32_t start = 0, off = 0, cnt = 0;
    if (col) { start = t.start[d]; off = t.off[d]; cnt = t.off[d + 1] - off; }
    // the source pixels this wavefront's outputs cover: starts and ends do not decrease with d
    const size_t d_first = tile_x * 64, d_last = d_first + 63 < dw ? d_first + 63 : dw - 1;
    const uint32_t lo = t.start[d_first];
    const uint32_t hi = t.start[d_last] + (t.off[d_last + 1] - t.off[d_last]);
    const size_t img_bytes = (size_t)sw * sh * BPP;
    for (size_t yb = tile_y * 4; yb < sh; yb += tiles_y * 4) {
        const size_t y = yb + threadIdx.y;
        const bool row = y < sh;
        uint32_t shift = 0;
        if (use_lds) {
            __syncthreads(); // (the segment of the previous round has been read)
            if (row) shift = stage_segment(src, img_bytes, (y * sw + lo) * BPP, (size_t)(hi - lo) * BPP, seg[threadIdx.y], threadIdx.x);
            __syncthreads();
        }
        if (!(row && col)) continue;
        float acc[BPP];
#pragma unroll
        for (int c = 0; c < BPP; ++c) acc[c] = 0.0f;
        if (use_lds) {
            const uint8_t *p = seg[threadIdx.y] + shift + (size_t)(start - lo) * BPP;
            for (uint32_t i = 0; i < cnt; ++i) {
                const float w = t.w[off + i];
#pragma unroll
                for (int c = 0; c < BPP; ++c) acc[c] = rz_tap(acc[c], p[(size_t)i * BPP + c], w);
            }
        } else {
            const uint8_t *p = src + (y * sw + start) * BPP;
            for (uint32_t i = 0; i < cnt; ++i) {
                const float w = t.w[off + i];
#pragma unroll
                for (int c = 0; c < BPP; ++c) acc[c] = rz_tap(acc[c], p[(size_t)i * BPP + c], w);
            }
        }
        uint8_t *out = mid + y * mid_stride + d * BPP; // (mid and its stride are 16-byte aligned)
        if (BPP == 4)
            *reinterpret_cast<uint32_t *>(out) = (uint32_t)rz_to_u8(acc[0]) | ((uint32_t)rz_to_u8(acc[1 % BPP]) << 8) |
                                                 ((uint32_t)rz_to_u8(acc[2 % BPP]) << 16) | ((uint32_t)rz_to_u8(acc[3 % BPP]) << 24);
        else if (BPP == 2)
            *reinterpret_cast<uint16_t *>(out) = (uint16_t)(rz_to_u8(acc[0]) | (rz_to_u8(acc[1 % BPP]) << 8));
        else
#pragma unroll
            for (int c = 0; c < BPP; ++c) out[c] = rz_to_u8(acc[c]);
    }
}
template <int BPP>
__global__ __launch_bounds__(256) void resize_lanczos_h_kernel(const uint8_t *__restrict__ src, uint32_t sw, uint32_t sh, uint8_t *__restrict__ mid,
                                                               size_t mid_stride, uint32_t dw, pixo_dev::ResizeAxisTable t, int use_lds)
{
    resize_lanczos_h_body<BPP>(src, sw, sh, mid, mid_stride, dw, t, use_lds, blockIdx.x, blockIdx.y, gridDim.y);
}
// One axis of the batch's tables (ResizeAxisTable's layout at a byte offset of the block)
__device__ __forceinline__ pixo_dev::ResizeAxisTable batch_axis(const uint8_t *tables, uint64_t at, uint32_t dst)
{
    pixo_dev::ResizeAxisTable t;
    t.start = reinterpret_cast<const uint32_t *>(tables + at);
    t.off = t.start + dst;
    t.w = reinterpret_cast<const float *>(t.off + dst + 1);
    return t;
}
// Image blockIdx.z of a sub-batch.  grid.y is sized for the tallest source: the body's row loop starts at blockIdx.y * 4, so a
// workgroup beyond its image's rows runs no round of it and meets no barrier; the loop's bounds are uniform over a workgroup.
template <int BPP>
__global__ __launch_bounds__(256) void resize_lanczos_h_batch_kernel(const pixo_dev::ResizeBatchItem *__restrict__ items,
                                                                     const uint8_t *__restrict__ tables, uint8_t *__restrict__ mid, size_t mid_stride,
                                                                     uint32_t dw)
{
    const pixo_dev::ResizeBatchItem it = items[blockIdx.z];
    resize_lanczos_h_body<BPP>(it.src, it.sw, it.sh, mid + it.mid_at, mid_stride, dw, batch_axis(tables, it.h_at, dw), (int)it.use_lds, blockIdx.x,
                               blockIdx.y, gridDim.y);
}
// Tile blockIdx.x of a ragged launch: 64 destination columns x 4 source rows of its image.  Record, tile and row stride are
// uniform over the workgroup, so the body's row loop — the one that holds the barriers — has the same bounds for all its
// threads; staged and direct images share a launch, use_lds is the image's.
template <int BPP>
__global__ __launch_bounds__(256) void resize_lanczos_h_images_kernel(const rzi::Record *__restrict__ records, uint32_t count,
                                                                      const uint8_t *__restrict__ tables, uint8_t *__restrict__ mid)
{
    const TileOf t = tile_of(records, count);
    resize_lanczos_h_body<BPP>(reinterpret_cast<const uint8_t *>(t.im->src), t.im->sw, t.im->sh, mid + t.im->mid_at, (size_t)t.im->mid_stride, t.im->dw,
                               batch_axis(tables, t.im->h_at, t.im->dw), (int)t.im->use_lds, t.tx, t.ty, t.im->tiles_y);
}

// ---- Lanczos3, vertical ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void resize_lanczos_v_body(const uint8_t *__restrict__ mid, size_t mid_stride, uint8_t *__restrict__ dst, size_t row_bytes,
                                                      uint32_t dh, pixo_dev::ResizeAxisTable t, size_t tile_x, size_t tile_y, size_t tiles_y)
{
    const size_t b = (tile_x * 256 + threadIdx.x) * 4;
    if (b >= row_bytes) return;
    const uint32_t n = row_bytes - b < 4 ? (uint32_t)(row_bytes - b) : 4;
    for (size_t y = tile_y; y < dh; y += tiles_y) {
        const uint32_t start = t.start[y], off = t.off[y], cnt = t.off[y + 1] - off; // uniform over the workgroup
        const uint8_t *p = mid + (size_t)start * mid_stride + b;                       // (b + 4 <= mid_stride: rows are padded)
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        for (uint32_t i = 0; i < cnt; ++i) {
            const float w = t.w[off + i];
            const uint32_t v = *reinterpret_cast<const uint32_t *>(p + (size_t)i * mid_stride);
            a0 = rz_tap(a0, (uint8_t)v, w);
            a1 = rz_tap(a1, (uint8_t)(v >> 8), w);
            a2 = rz_tap(a2, (uint8_t)(v >> 16), w);
            a3 = rz_tap(a3, (uint8_t)(v >> 24), w);
        }
        const uint8_t o[4] = {rz_to_u8(a0), rz_to_u8(a1), rz_to_u8(a2), rz_to_u8(a3)};
        uint8_t *out = dst + y * row_bytes + b;
        if (n == 4 && (reinterpret_cast<uintptr_t>(out) & 3) == 0)
            *reinterpret_cast<uint32_t *>(out) = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
        else
            for (uint32_t k = 0; k < n; ++k) out[k] = o[k];
    }
}
__global__ __launch_bounds__(256) void resize_lanczos_v_kernel(const uint8_t *__restrict__ mid, size_t mid_stride, uint8_t *__restrict__ dst,
                                                               size_t row_bytes, uint32_t dh, pixo_dev::ResizeAxisTable t)
{
    resize_lanczos_v_body(mid, mid_stride, dst, row_bytes, dh, t, blockIdx.x, blockIdx.y, gridDim.y);
}
// Image blockIdx.z of a sub-batch: its vertical table, its rows of the intermediate (mid_at is a multiple of 16: rows are padded)
__global__ __launch_bounds__(256) void resize_lanczos_v_batch_kernel(const pixo_dev::ResizeBatchItem *__restrict__ items,
                                                                     const uint8_t *__restrict__ tables, const uint8_t *__restrict__ mid,
                                                                     size_t mid_stride, uint8_t *__restrict__ dst, size_t row_bytes, uint32_t dh)
{
    const pixo_dev::ResizeBatchItem it = items[blockIdx.z];
    resize_lanczos_v_body(mid + it.mid_at, mid_stride, dst + (size_t)blockIdx.z * row_bytes * dh, row_bytes, dh, batch_axis(tables, it.v_at, dh),
                          blockIdx.x, blockIdx.y, gridDim.y);
}
// Tile blockIdx.x of a ragged launch: 1024 bytes of one destination row of its image, whatever its pixel size: one launch
// serves every image of a sub-batch.
__global__ __launch_bounds__(256) void resize_lanczos_v_images_kernel(const rzi::Record *__restrict__ records, uint32_t count,
                                                                      const uint8_t *__restrict__ tables, const uint8_t *__restrict__ mid)
{
    const TileOf t = tile_of(records, count);
    resize_lanczos_v_body(mid + t.im->mid_at, (size_t)t.im->mid_stride, reinterpret_cast<uint8_t *>(t.im->dst), (size_t)t.im->dw * t.im->bpp, t.im->dh,
                          batch_axis(tables, t.im->v_at, t.im->dh), t.tx, t.ty, t.im->tiles_y);
}

uint32_t rows_grid(uint32_t rows, uint32_t per_block) // grid.y: the kernels stride over what does not fit
{
    const uint32_t g = (rows + per_block - 1) / per_block;
    return g < rzi::kRowsCap ? g : rzi::kRowsCap; // (65535: the images entries cap an image's rows of tiles at the same value)
}

} // namespace

namespace pixo_dev {

hipError_t launch_resize_point(const uint8_t *d_src, uint32_t sw, uint32_t sh, uint8_t *d_dst, uint32_t dw, uint32_t dh, uint32_t bpp,
                               int algorithm, hipStream_t stream)
{
    if (bpp < 1 || bpp > 4 || (algorithm != RZ_NEAREST && algorithm != RZ_BILINEAR)) return hipErrorInvalidValue;
    const dim3 grid((dw + 255) / 256, rows_grid(dh, 4)), block(64, 4);
#define PIXO_RZ_POINT(B, A) hipLaunchKernelGGL((resize_point_kernel<B, A>), grid, block, 0, stream, d_src, sw, sh, d_dst, dw, dh)
    if (algorithm == RZ_NEAREST) {
        switch (bpp) {
        case 1: PIXO_RZ_POINT(1, RZ_NEAREST); break;
        case 2: PIXO_RZ_POINT(2, RZ_NEAREST); break;
        case 3: PIXO_RZ_POINT(3, RZ_NEAREST); break;
        default: PIXO_RZ_POINT(4, RZ_NEAREST); break;
        }
    } else {
        switch (bpp) {
        case 1: PIXO_RZ_POINT(1, RZ_BILINEAR); break;
        case 2: PIXO_RZ_POINT(2, RZ_BILINEAR); break;
        case 3: PIXO_RZ_POINT(3, RZ_BILINEAR); break;
        default: PIXO_RZ_POINT(4, RZ_BILINEAR); break;
        }
    }
#undef PIXO_RZ_POINT
    return hipGetLastError();
}

hipError_t launch_resize_lanczos_h(const uint8_t *d_src, uint32_t sw, uint32_t sh, uint8_t *d_mid, uint32_t dw, uint32_t bpp,
                                   ResizeAxisTable t, uint32_t max_span, hipStream_t stream)
{
    if (bpp < 1 || bpp > 4) return hipErrorInvalidValue;
    static_assert(kResizeHTile == 64, "a wavefront per tile");
    // the staged segment keeps the source's alignment (up to 3 bytes in front) and is stored in whole dwords
    const int use_lds = resize_h_uses_lds(max_span, bpp);
    const size_t stride = resize_mid_stride(dw, bpp);
    const dim3 grid((dw + 63) / 64, rows_grid(sh, 4)), block(64, 4);
#define PIXO_RZ_H(B) hipLaunchKernelGGL((resize_lanczos_h_kernel<B>), grid, block, 0, stream, d_src, sw, sh, d_mid, stride, dw, t, use_lds)
    switch (bpp) {
    case 1: PIXO_RZ_H(1); break;
    case 2: PIXO_RZ_H(2); break;
    case 3: PIXO_RZ_H(3); break;
    default: PIXO_RZ_H(4); break;
    }
#undef PIXO_RZ_H
    return hipGetLastError();
}

hipError_t launch_resize_lanczos_v(const uint8_t *d_mid, uint32_t sh, uint8_t *d_dst, uint32_t dw, uint32_t dh, uint32_t bpp,
                                   ResizeAxisTable t, hipStream_t stream)
{
    (void)sh;
    const size_t row_bytes = static_cast<size_t>(dw) * bpp;
    const dim3 grid(static_cast<unsigned>((row_bytes + 1023) / 1024), rows_grid(dh, 1)), block(256);
    hipLaunchKernelGGL(resize_lanczos_v_kernel, grid, block, 0, stream, d_mid, resize_mid_stride(dw, bpp), d_dst, row_bytes, dh, t);
    return hipGetLastError();
}

hipError_t launch_resize_point_batch(const ResizeBatchItem *d_items, uint32_t n, uint8_t *d_dst, uint32_t dw, uint32_t dh, uint32_t bpp,
                                     int algorithm, hipStream_t stream)
{
    if (bpp < 1 || bpp > 4 || n < 1 || n > 65535 || (algorithm != RZ_NEAREST && algorithm != RZ_BILINEAR)) return hipErrorInvalidValue;
    const dim3 grid((dw + 255) / 256, rows_grid(dh, 4), n), block(64, 4);
#define PIXO_RZ_POINT(B, A) hipLaunchKernelGGL((resize_point_batch_kernel<B, A>), grid, block, 0, stream, d_items, d_dst, dw, dh)
    if (algorithm == RZ_NEAREST) {
        switch (bpp) {
        case 1: PIXO_RZ_POINT(1, RZ_NEAREST); break;
        case 2: PIXO_RZ_POINT(2, RZ_NEAREST); break;
        case 3: PIXO_RZ_POINT(3, RZ_NEAREST); break;
        default: PIXO_RZ_POINT(4, RZ_NEAREST); break;
        }
    } else {
        switch (bpp) {
        case 1: PIXO_RZ_POINT(1, RZ_BILINEAR); break;
        case 2: PIXO_RZ_POINT(2, RZ_BILINEAR); break;
        case 3: PIXO_RZ_POINT(3, RZ_BILINEAR); break;
        default: PIXO_RZ_POINT(4, RZ_BILINEAR); break;
        }
    }
#undef PIXO_RZ_POINT
    return hipGetLastError();
}

hipError_t launch_resize_lanczos_h_batch(const ResizeBatchItem *d_items, uint32_t n, uint32_t max_sh, const uint8_t *d_tables, uint8_t *d_mid,
                                         uint32_t dw, uint32_t bpp, hipStream_t stream)
{
    if (bpp < 1 || bpp > 4 || n < 1 || n > 65535) return hipErrorInvalidValue;
    const size_t stride = resize_mid_stride(dw, bpp);
    const dim3 grid((dw + 63) / 64, rows_grid(max_sh, 4), n), block(64, 4);
#define PIXO_RZ_H(B) hipLaunchKernelGGL((resize_lanczos_h_batch_kernel<B>), grid, block, 0, stream, d_items, d_tables, d_mid, stride, dw)
    switch (bpp) {
    case 1: PIXO_RZ_H(1); break;
    case 2: PIXO_RZ_H(2); break;
    case 3: PIXO_RZ_H(3); break;
    default: PIXO_RZ_H(4); break;
    }
#undef PIXO_RZ_H
    return hipGetLastError();
}

hipError_t launch_resize_lanczos_v_batch(const ResizeBatchItem *d_items, uint32_t n, const uint8_t *d_tables, const uint8_t *d_mid, uint8_t *d_dst,
                                         uint32_t dw, uint32_t dh, uint32_t bpp, hipStream_t stream)
{
    if (n < 1 || n > 65535) return hipErrorInvalidValue;
    const size_t row_bytes = static_cast<size_t>(dw) * bpp;
    const dim3 grid(static_cast<unsigned>((row_bytes + 1023) / 1024), rows_grid(dh, 1), n), block(256);
    hipLaunchKernelGGL(resize_lanczos_v_batch_kernel, grid, block, 0, stream, d_items, d_tables, d_mid, resize_mid_stride(dw, bpp), d_dst, row_bytes,
                       dh);
    return hipGetLastError();
}

hipError_t launch_resize_point_images(const pixo_resize_images::Record *d_records, uint32_t count, uint32_t tiles, uint32_t bpp, int algorithm,
                                      hipStream_t stream)
{
    if (bpp < 1 || bpp > 4 || count < 1 || tiles < count || tiles > rzi::kMaxTiles || (algorithm != RZ_NEAREST && algorithm != RZ_BILINEAR))
        return hipErrorInvalidValue;
    const dim3 grid(tiles), block(64, 4);
#define PIXO_RZ_POINT(B, A) hipLaunchKernelGGL((resize_point_images_kernel<B, A>), grid, block, 0, stream, d_records, count)
    if (algorithm == RZ_NEAREST) {
        switch (bpp) {
        case 1: PIXO_RZ_POINT(1, RZ_NEAREST); break;
        case 2: PIXO_RZ_POINT(2, RZ_NEAREST); break;
        case 3: PIXO_RZ_POINT(3, RZ_NEAREST); break;
        default: PIXO_RZ_POINT(4, RZ_NEAREST); break;
        }
    } else {
        switch (bpp) {
        case 1: PIXO_RZ_POINT(1, RZ_BILINEAR); break;
        case 2: PIXO_RZ_POINT(2, RZ_BILINEAR); break;
        case 3: PIXO_RZ_POINT(3, RZ_BILINEAR); break;
        default: PIXO_RZ_POINT(4, RZ_BILINEAR); break;
        }
    }
#undef PIXO_RZ_POINT
    return hipGetLastError();
}

hipError_t launch_resize_lanczos_h_images(const pixo_resize_images::Record *d_records, uint32_t count, uint32_t tiles, const uint8_t *d_tables,
                                          uint8_t *d_mid, uint32_t bpp, hipStream_t stream)
{
    if (bpp < 1 || bpp > 4 || count < 1 || tiles < count || tiles > rzi::kMaxTiles) return hipErrorInvalidValue;
    const dim3 grid(tiles), block(64, 4);
#define PIXO_RZ_H(B) hipLaunchKernelGGL((resize_lanczos_h_images_kernel<B>), grid, block, 0, stream, d_records, count, d_tables, d_mid)
    switch (bpp) {
    case 1: PIXO_RZ_H(1); break;
    case 2: PIXO_RZ_H(2); break;
    case 3: PIXO_RZ_H(3); break;
    default: PIXO_RZ_H(4); break;
    }
#undef PIXO_RZ_H
    return hipGetLastError();
}

hipError_t launch_resize_lanczos_v_images(const pixo_resize_images::Record *d_records, uint32_t count, uint32_t tiles, const uint8_t *d_tables,
                                          const uint8_t *d_mid, hipStream_t stream)
{
    if (count < 1 || tiles < count || tiles > rzi::kMaxTiles) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resize_lanczos_v_images_kernel, dim3(tiles), dim3(256), 0, stream, d_records, count, d_tables, d_mid);
    return hipGetLastError();
}

} // namespace pixo_dev
