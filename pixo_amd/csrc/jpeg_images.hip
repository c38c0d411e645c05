// jpeg_images.hip — the RAGGED coefficient kernel: images of individual sizes, anywhere in device memory, in one flat launch
// per class (mode x load form) of a sub-batch (jpeg_images_api.cpp).  A workgroup is one 512-pixel tile, as in jpeg_kernels.hip;
// what differs is where it learns which image it belongs to: a binary search over a table of 40-byte records
// (jpeg_images_math.h) by its flat tile index.  The index is uniform across the workgroup and the table is read through the
// constant address space, so the search and the record are scalar loads and everything they yield stays in scalar registers.
// The tile body is jpeg_tile.h's, unchanged: phase A (pixels -> planar LDS), one LDS barrier, phase B (DCT, quantiser, stores).
//
// Every vector load of phase A is clamped to the image's own last 4-pixel group and last row (lane_addr, producer_load_item):
// a tile never reads a byte outside [px, px + W * H * bpp), whatever lies around the image.
//
// Not taken over from the single entry's kernel: the preloaded kernel arguments (the record is what a workgroup waits for
// here) and the late start of half a generation (tuned for one 4096x4096 image whose tiles all arrive at once).
#include <hip/hip_runtime.h>

#include "capi_internal.hpp" // (route record)
#include "jpeg_images.hpp"
#include "jpeg_kernels.hpp"
#include "jpeg_tile.h"

#pragma clang fp contract(off)

namespace pixo_dev {
using namespace pixo_tile;
namespace ji = pixo_jpeg_images;

static_assert((int)M420 == ji::MODE_420 && (int)M444 == ji::MODE_444 && (int)MGRAY == ji::MODE_GRAY, "jpeg_images_math.h names the tile body's modes");
static_assert((int)L_BYTES == ji::LOAD_BYTES && (int)L_ALIGNED == ji::LOAD_ALIGNED && (int)L_FUNNEL == ji::LOAD_FUNNEL, "... and its load forms");

namespace {
using ConstTile = const __attribute__((address_space(4))) ji::TileRecord;

// Workgroup barrier that orders LDS only (jpeg_kernels.hip: __syncthreads() would also wait for the stores)
__device__ __forceinline__ void lds_barrier_images()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Phase A of one wavefront: COUNT items [first, first + COUNT) of the tile, HBM -> registers -> planar LDS; all loads are
// issued before the first conversion.
template <int MODE, int LOAD, int COUNT>
__device__ __forceinline__ void phase_a_images(const TileCtx &c, uint32_t tx, uint32_t ty, int first, int lane, uint8_t *lds)
{
    typedef Geo<MODE> G;
    uint32_t r[COUNT * G::item_regs];
    LaneAddr la{};
    if (LOAD != L_BYTES) la = lane_addr<MODE>(c, tx, ty, lane);
#pragma unroll
    for (int j = 0; j < COUNT; j++) producer_load_item<MODE, LOAD>(c, la, tx, ty, first + j, lane, &r[j * G::item_regs]);
#pragma unroll
    for (int j = 0; j < COUNT; j++) {
        producer_fix_item<MODE, LOAD>(c, tx, first + j, lane, &r[j * G::item_regs]);
        producer_color_item<MODE, LOAD != L_BYTES>(first + j, lane, &r[j * G::item_regs], lds);
    }
}

template <int MODE, int LOAD, bool PACKED>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(6, 6))) void jpeg_images_coeffs_kernel(const ji::TileRecord *records, uint32_t count,
                                                                                                             int16_t *tuple, const float *qt)
{
    typedef Geo<MODE> G;
    __shared__ __attribute__((aligned(16))) uint8_t lds[G::planar];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    ConstTile *table = (ConstTile *)records;
    ConstTile *im = table + ji::image_of_tile(table, count, blockIdx.x);
    const uint32_t t = blockIdx.x - im->first_tile, tiles_x = im->tiles_x;
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    TileCtx c;
    c.px = reinterpret_cast<const uint8_t *>(im->px);
    c.y = c.cb = c.cr = nullptr;
    c.qt = qt;
    c.W = im->wh & 0xFFFFu; c.H = im->wh >> 16;
    c.units_x = im->units & 0xFFFFu; c.units_y = im->units >> 16;
    c.fast = LOAD != L_BYTES;
    c.px_end = c.px + (size_t)c.W * c.H * (uint32_t)G::bpp; // the image's own last byte: nothing is read at or behind it
    __builtin_amdgcn_s_setprio(1); // (phase A at raised priority, as in jpeg_kernels.hip)
    constexpr int base = G::items / kWaves, extra = G::items % kWaves;
    const int first = (extra && wave < extra) ? wave * (base + 1) : extra * (base + 1) + (wave - extra) * base;
    if (extra && wave < extra) phase_a_images<MODE, LOAD, base + 1>(c, tx, ty, first, lane, lds);
    else phase_a_images<MODE, LOAD, base>(c, tx, ty, first, lane, lds);
    lds_barrier_images();
    __builtin_amdgcn_s_setprio(0);
    c.y = tuple + (size_t)im->y_block * 64;
    if (MODE != MGRAY) {
        c.cb = tuple + (size_t)im->cb_block * 64;
        c.cr = tuple + (size_t)im->cr_block * 64;
    }
    float v[64];
    consumer_rows<MODE, PACKED>(wave, lane, lds, v);
    consumer_cols<PACKED>(v);
    uint8_t *stage = lds + stage_offset<MODE>(wave); // inside this wavefront's own planar area
    uint32_t qw[32];
    consumer_quant<MODE, PACKED>(wave, lane, qt, v, qw);
#pragma unroll
    for (int h = 0; h < 2; h++) {
        consumer_stage_blocks(lane, h, qw, stage);
        consumer_stage_sync();
        consumer_store_blocks<MODE>(c, tx, ty, wave, lane, h, stage);
        consumer_stage_sync();
    }
}

template <int MODE, int LOAD>
hipError_t launch_form(const ji::TileRecord *d_records, uint32_t count, uint32_t tiles, int16_t *d_tuple, const float *d_qt, hipStream_t s)
{
    // one generation of workgroups: the scalar forms of the DCT passes and the quantiser; more: the packed ones (packed_launch)
    if (packed_launch(tiles)) hipLaunchKernelGGL((jpeg_images_coeffs_kernel<MODE, LOAD, true>), dim3(tiles), dim3(kThreads), 0, s, d_records, count, d_tuple, d_qt);
    else hipLaunchKernelGGL((jpeg_images_coeffs_kernel<MODE, LOAD, false>), dim3(tiles), dim3(kThreads), 0, s, d_records, count, d_tuple, d_qt);
    return hipGetLastError();
}
template <int MODE>
hipError_t launch_load(int load, const ji::TileRecord *d_records, uint32_t count, uint32_t tiles, int16_t *d_tuple, const float *d_qt, hipStream_t s)
{
    namespace r = pixo_capi::route;
    pixo_capi::note_route(load == L_ALIGNED ? r::LOAD_ALIGNED : (load == L_FUNNEL ? r::LOAD_FUNNEL : r::LOAD_BYTES));
    if (load == L_ALIGNED) return launch_form<MODE, L_ALIGNED>(d_records, count, tiles, d_tuple, d_qt, s);
    if (load == L_FUNNEL) return launch_form<MODE, L_FUNNEL>(d_records, count, tiles, d_tuple, d_qt, s);
    return launch_form<MODE, L_BYTES>(d_records, count, tiles, d_tuple, d_qt, s);
}
} // namespace

hipError_t launch_jpeg_images_coeffs(int mode, int load, const ji::TileRecord *d_records, uint32_t count, uint32_t tiles, int16_t *d_tuple,
                                     const float *d_qt, hipStream_t stream)
{
    if (count == 0 || tiles == 0 || tiles > 0x7FFFFFFFu || load < 0 || load > 2) return hipErrorInvalidValue;
    if (mode == ji::MODE_GRAY) return launch_load<MGRAY>(load, d_records, count, tiles, d_tuple, d_qt, stream);
    if (mode == ji::MODE_420) return launch_load<M420>(load, d_records, count, tiles, d_tuple, d_qt, stream);
    if (mode == ji::MODE_444) return launch_load<M444>(load, d_records, count, tiles, d_tuple, d_qt, stream);
    return hipErrorInvalidValue;
}

} // namespace pixo_dev
