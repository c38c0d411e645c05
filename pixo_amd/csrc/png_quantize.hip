// png_quantize.hip — PNG palette quantisation on the device (gfx950): the parts of quantize_image (src/png/mod.rs:1505-1701)
// that touch every pixel, every histogram colour or every cell of the 64^3 table.  The arithmetic is png_quantize_math.h.
//
//   gather   the strided samples the gate (should_quantize_auto) and the histogram are made from, as colour keys
//   assign   a k-means round: a thread per histogram colour, palette in LDS, u64 sums in LDS, one global add per touched word
//   lut      PaletteLut::new: 262,144 cells x n entries.  A thread makes the four cells (r6, g6, 4k .. 4k + 3): they share the
//            red and green terms of every distance, an entry is ONE 16-byte LDS read that all lanes make at the same address
//            (a broadcast), the factors are masked to the bits they can have so that the squares and the red term are
//            full-rate 24-bit multiplies (the four blue multiply-adds per entry still compile to v_mad_u64_u32), the
//            minimum is a v_min_u32 over distance << 8 | index (the first minimum wins), and a wavefront stores 256
//            consecutive bytes as dwords.
//   map      pixel -> index without dithering: four pixels per thread, one dword stored
//   dither   Floyd-Steinberg on the skewed wavefront.  A band is 64 rows, a row per lane; at step s lane l is at x = s - 2l,
//            so the sum it needs from the row above was completed one step earlier by lane l - 1 and arrives by one lane
//            shuffle per channel; W + 126 steps per band.  A band's last row leaves its sums for the first row of the band
//            below in HBM, one 8-byte word per column that carries its own "written" bit (agent-scope atomic store, agent-scope atomic
//            load: no fence on the dependent path).  Chained: all bands in one launch, each takes its band from a ticket
//            (so the band above has started) and polls a column's word at most spin_budget times; a band that gives up says
//            so and every other band follows.  Band by band: the same kernel, one band per launch in stream order; every
//            word it reads was written by an earlier launch.  Dependent steps: W + 2H, against the reference's W * H.
// Bounds: every kernel's indices are below the element counts its launcher was given; the dither kernel reads and writes
// rows < height and columns < width only, carry lines 1 .. bands - 1 of `bands` lines.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "png_quantize.hpp"

namespace pixo_dev {
using namespace pixo_pngq;

namespace {
constexpr int kThreads = 256;
constexpr uint64_t kMaxBlocks = 2048;

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned int gu32;

uint32_t blocks_for(uint64_t items) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kMaxBlocks, (items + kThreads - 1) / kThreads)); }

__global__ __launch_bounds__(kThreads) void pngq_gather_kernel(const uint8_t *px, uint32_t spp, uint64_t stride_a, uint32_t count_a,
                                                               uint64_t stride_b, uint32_t count_b, uint32_t *keys)
{
    const uint32_t total = count_a + count_b;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < total; i += gridDim.x * kThreads) {
        const uint64_t pixel = i < count_a ? i * stride_a : (uint64_t)(i - count_a) * stride_b;
        keys[i] = color_key(px + pixel * spp, spp);
    }
}

__global__ __launch_bounds__(kThreads) void pngq_assign_kernel(const uint32_t *colors, const uint32_t *counts, uint32_t n_colors,
                                                               const uint32_t *palette, uint32_t n, unsigned long long *acc)
{
    __shared__ uint32_t pal[kMaxPalette];
    __shared__ unsigned long long sums[kMaxPalette * 5];
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) pal[i] = palette[i];
    for (uint32_t i = threadIdx.x; i < n * 5; i += kThreads) sums[i] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n_colors) {
        const uint32_t c = colors[i];
        const unsigned long long cnt = counts[i];
        unsigned long long *s = sums + 5 * nearest(pal, n, c);
        atomicAdd(s + 0, (c >> 24) * cnt);
        atomicAdd(s + 1, ((c >> 16) & 255) * cnt);
        atomicAdd(s + 2, ((c >> 8) & 255) * cnt);
        atomicAdd(s + 3, (c & 255) * cnt);
        atomicAdd(s + 4, cnt);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n * 5; k += kThreads)
        if (sums[k]) atomicAdd(acc + k, sums[k]);
}

__global__ __launch_bounds__(kThreads) void pngq_lut_kernel(const uint32_t *palette, uint32_t n, uint32_t *lut_words)
{
    __shared__ __attribute__((aligned(16))) int4 pal[kMaxPalette]; // r, g, b, (255 - a)^2
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
        const uint32_t p = palette[i];
        const int da = 255 - (int)(p & 255);
        pal[i] = make_int4((int)(p >> 24), (int)((p >> 16) & 255), (int)((p >> 8) & 255), da * da);
    }
    __syncthreads();
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x; // < kLutCells / 4: the grid is exact
    const int r8 = (int)expand6(t >> 10), g8 = (int)expand6((t >> 4) & 63);
    int b8[4];
    uint32_t best[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        b8[c] = (int)expand6((t & 15) * 4 + c);
        best[c] = 0xFFFFFFFFu;
    }
#pragma unroll 4
    for (uint32_t i = 0; i < n; ++i) {
        const int4 p = pal[i];
        // Every factor is masked to the bits it can have (differences as magnitudes below 256, weights below 1024), so that
        // the 24-bit multiplies are provably exact; every product stays below 2^28.
        const uint32_t pr = (uint32_t)p.x & 255u, dr = (uint32_t)abs(r8 - (int)pr) & 255u, dg = (uint32_t)abs(g8 - (p.y & 255)) & 255u;
        const uint32_t r_mean = ((uint32_t)r8 + pr) >> 1;
        const uint32_t rg = (uint32_t)__mul24((int)((512u + r_mean) & 1023u), (int)__umul24(dr, dr)) + (__umul24(dg, dg) << 10), bw = (767u - r_mean) & 1023u;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t db = (uint32_t)abs(b8[c] - (p.z & 255)) & 255u;
            const uint32_t d = ((uint32_t)((int)rg + __mul24((int)bw, (int)__umul24(db, db))) >> 8) + (uint32_t)p.w;
            best[c] = min(best[c], (d << 8) | i);
        }
    }
    lut_words[t] = (best[0] & 255u) | ((best[1] & 255u) << 8) | ((best[2] & 255u) << 16) | ((best[3] & 255u) << 24);
}

template <bool ALIGNED4>
__global__ __launch_bounds__(kThreads) void pngq_map_kernel(const uint8_t *px, uint64_t pixels, uint32_t spp, const uint8_t *lut,
                                                            const uint32_t *palette, uint32_t n, uint8_t *index)
{
    __shared__ uint32_t pal[kMaxPalette];
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) pal[i] = palette[i];
    __syncthreads();
    const uint64_t groups = (pixels + 3) / 4;
    for (uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * kThreads) {
        const uint64_t first = 4 * g;
        const uint32_t valid = pixels - first >= 4 ? 4u : (uint32_t)(pixels - first);
        uint32_t out = 0;
        for (uint32_t k = 0; k < valid; ++k) {
            uint32_t key;
            if (ALIGNED4) key = __builtin_bswap32(reinterpret_cast<const uint32_t *>(px)[first + k]); // bytes r g b a -> r<<24 | ... | a
            else key = color_key(px + (first + k) * spp, spp);
            const uint32_t idx = (lut && (key & 255u) == 255u) ? lut[cell_of(key >> 24, (key >> 16) & 255, (key >> 8) & 255)] : nearest(pal, n, key);
            out |= idx << (8 * k);
        }
        if (valid == 4) reinterpret_cast<uint32_t *>(index)[g] = out; // (the index image is the context's own buffer, never a caller's: launch_pngq_map refuses one that is not 4-byte aligned)
        else
            for (uint32_t k = 0; k < valid; ++k) index[first + k] = (uint8_t)(out >> (8 * k));
    }
}

// A pixel as it comes from memory, untouched until the step that uses it: nothing waits for the load in the step that issues it.
template <bool ALIGNED4> struct RawPixel;
template <> struct RawPixel<true> { // RGBA at a 4-byte aligned address: one dword
    uint32_t w;
    __device__ __forceinline__ void load(const uint8_t *px, uint32_t, uint64_t pixel) { w = reinterpret_cast<const uint32_t *>(px)[pixel]; }
    __device__ __forceinline__ uint32_t key(uint32_t) const { return __builtin_bswap32(w); }
};
template <> struct RawPixel<false> {
    uint8_t r, g, b, a;
    __device__ __forceinline__ void load(const uint8_t *px, uint32_t spp, uint64_t pixel)
    {
        const uint8_t *p = px + pixel * spp;
        r = p[0]; g = p[1]; b = p[2];
        a = p[spp - 1]; // (RGB: blue again, not used)
    }
    __device__ __forceinline__ uint32_t key(uint32_t spp) const { return ((uint32_t)r << 24) | ((uint32_t)g << 16) | ((uint32_t)b << 8) | (spp == 4 ? (uint32_t)a : 255u); }
};

template <bool ALIGNED4>
__global__ __launch_bounds__(64) void pngq_dither_kernel(const DitherArgs a, const uint32_t chained, const uint32_t only_band, const uint32_t spin_budget)
{
    __shared__ uint32_t pal[kMaxPalette];
    const int lane = (int)threadIdx.x;
    gu32 *state = (gu32 *)a.state;
    uint32_t band = only_band;
    if (chained) {
        uint32_t ticket = 0;
        if (lane == 0) ticket = __hip_atomic_fetch_add(state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        band = (uint32_t)__shfl((int)ticket, 0);
    }
    for (uint32_t i = (uint32_t)lane; i < a.n; i += 64) pal[i] = a.palette[i];
    __syncthreads();

    const int64_t W = a.width;
    const uint32_t row0 = band * kBandRows;
    if (row0 >= a.height) return;
    const uint32_t rows = min(kBandRows, a.height - row0);
    const bool active_row = (uint32_t)lane < rows, has_above = band > 0, has_below = row0 + kBandRows < a.height;
    const uint64_t row_at = (uint64_t)(row0 + (active_row ? lane : 0)) * a.width;
    gu64 *in_carry = (gu64 *)a.carry + (uint64_t)band * a.width;
    gu64 *out_carry = (gu64 *)a.carry + (uint64_t)(band + 1) * a.width; // (stored to only when has_below: then band + 1 < bands)
    const bool takes = lane == 0 && has_above, leaves = lane == (int)kBandRows - 1 && has_below;

    int ea[3] = {0, 0, 0}, eb[3] = {0, 0, 0}, below[3] = {0, 0, 0};
    // What the next step needs from memory is asked for one step ahead and kept as loaded.  The pixel's load is unconditional:
    // its column is clamped into the row, so it never leaves the image (a row that does not exist reads the band's first).
    int64_t x = -2 * (int64_t)lane;
    RawPixel<ALIGNED4> px_next;
    px_next.load(a.px, a.spp, row_at);
    uint64_t carry_next = (takes && x == 0) ? __hip_atomic_load(in_carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    const int64_t steps = W + 2 * (int64_t)(rows - 1) + 1;
    for (int64_t s = 0; s < steps; ++s, ++x) {
        int up[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) up[k] = __shfl_up(below[k], 1);
        const bool in_row = x >= 0 && x < W, here = active_row && in_row;
        const RawPixel<ALIGNED4> px_now = px_next;
        uint64_t carry = carry_next;
        px_next.load(a.px, a.spp, row_at + (uint64_t)min(max(x + 1, (int64_t)0), W - 1));
        if (takes && x + 1 < W) carry_next = __hip_atomic_load(in_carry + (x + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool dead = false;
        if (lane == 0) {
            up[0] = up[1] = up[2] = 0;
            if (takes && in_row) {
                uint32_t polls = 0;
                while (!(carry & kCarryValid)) {
                    if (++polls > spin_budget || ((polls & 255u) == 0 && __hip_atomic_load(state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                        dead = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                    carry = __hip_atomic_load(in_carry + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (dead) __hip_atomic_store(state + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else unpack_carry(carry, &up[0], &up[1], &up[2]);
            }
        }
        if (__any(dead)) return; // (the whole band: nothing below it can finish either, and says so itself)
        int e[3] = {0, 0, 0};
        if (here) {
            const uint32_t key = px_now.key(a.spp);
            const int32_t c[4] = {(int32_t)(key >> 24), (int32_t)((key >> 16) & 255), (int32_t)((key >> 8) & 255), (int32_t)(key & 255)};
            const int32_t in16[3] = {up[0] + 7 * ea[0], up[1] + 7 * ea[1], up[2] + 7 * ea[2]};
            a.index[row_at + (uint64_t)x] = (uint8_t)dither_pixel(a.lut, pal, a.n, c, in16, e);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            below[k] = dither_below(eb[k], ea[k], e[k]); // for column x - 1 of the row below
            eb[k] = ea[k];
            ea[k] = e[k];
        }
        if (leaves && x >= 1 && x <= W)
            __hip_atomic_store(out_carry + (x - 1), (unsigned long long)pack_carry(below[0], below[1], below[2]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

} // namespace

hipError_t launch_pngq_gather(const void *d_pixels, uint32_t spp, uint64_t stride_a, uint32_t count_a, uint64_t stride_b, uint32_t count_b,
                              uint32_t *d_keys, hipStream_t stream)
{
    if ((spp != 3 && spp != 4) || count_a + count_b == 0) return hipErrorInvalidValue;
    pngq_gather_kernel<<<blocks_for(count_a + count_b), kThreads, 0, stream>>>(static_cast<const uint8_t *>(d_pixels), spp, stride_a, count_a, stride_b,
                                                                                count_b, d_keys);
    return hipGetLastError();
}

hipError_t launch_pngq_assign(const uint32_t *d_colors, const uint32_t *d_counts, uint32_t n_colors, const uint32_t *d_palette, uint32_t n,
                              unsigned long long *d_acc, hipStream_t stream)
{
    if (n == 0 || n > kMaxPalette || n_colors == 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_acc, 0, kMaxPalette * 5 * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    pngq_assign_kernel<<<(n_colors + kThreads - 1) / kThreads, kThreads, 0, stream>>>(d_colors, d_counts, n_colors, d_palette, n, d_acc);
    return hipGetLastError();
}

hipError_t launch_pngq_lut(const uint32_t *d_palette, uint32_t n, uint8_t *d_lut, hipStream_t stream)
{
    if (n == 0 || n > kMaxPalette) return hipErrorInvalidValue;
    static_assert(kLutCells / 4 % kThreads == 0, "the grid covers the table exactly");
    pngq_lut_kernel<<<kLutCells / 4 / kThreads, kThreads, 0, stream>>>(d_palette, n, reinterpret_cast<uint32_t *>(d_lut));
    return hipGetLastError();
}

hipError_t launch_pngq_map(const void *d_pixels, uint64_t pixels, uint32_t spp, const uint8_t *d_lut, const uint32_t *d_palette, uint32_t n,
                           uint8_t *d_index, hipStream_t stream)
{
    if ((spp != 3 && spp != 4) || n == 0 || n > kMaxPalette || pixels == 0) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(d_index) % 4) return hipErrorInvalidValue; // four indices a store; the pixels may sit anywhere
    const uint8_t *px = static_cast<const uint8_t *>(d_pixels);
    const uint32_t blocks = blocks_for((pixels + 3) / 4);
    if (spp == 4 && reinterpret_cast<uintptr_t>(px) % 4 == 0) pngq_map_kernel<true><<<blocks, kThreads, 0, stream>>>(px, pixels, spp, d_lut, d_palette, n, d_index);
    else pngq_map_kernel<false><<<blocks, kThreads, 0, stream>>>(px, pixels, spp, d_lut, d_palette, n, d_index);
    return hipGetLastError();
}

namespace {
bool dither_aligned4(const DitherArgs &a) { return a.spp == 4 && reinterpret_cast<uintptr_t>(a.px) % 4 == 0; }
bool dither_args_ok(const DitherArgs &a) { return (a.spp == 3 || a.spp == 4) && a.width && a.height && a.n && a.n <= kMaxPalette; }
} // namespace

hipError_t launch_pngq_dither_chained(const DitherArgs &a, uint32_t spin_budget, hipStream_t stream)
{
    if (!dither_args_ok(a)) return hipErrorInvalidValue;
    const uint32_t bands = (a.height + kBandRows - 1) / kBandRows;
    hipError_t e = hipMemsetAsync(a.state, 0, kDitherStateWords * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.carry, 0, (size_t)bands * a.width * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    if (dither_aligned4(a)) pngq_dither_kernel<true><<<bands, 64, 0, stream>>>(a, 1u, 0u, spin_budget);
    else pngq_dither_kernel<false><<<bands, 64, 0, stream>>>(a, 1u, 0u, spin_budget);
    return hipGetLastError();
}

hipError_t launch_pngq_dither_band(const DitherArgs &a, uint32_t only_band, hipStream_t stream)
{
    if (!dither_args_ok(a) || (uint64_t)only_band * kBandRows >= a.height) return hipErrorInvalidValue;
    if (only_band == 0) {
        const hipError_t e = hipMemsetAsync(a.state, 0, kDitherStateWords * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
    }
    if (dither_aligned4(a)) pngq_dither_kernel<true><<<1, 64, 0, stream>>>(a, 0u, only_band, 0u);
    else pngq_dither_kernel<false><<<1, 64, 0, stream>>>(a, 0u, only_band, 0u);
    return hipGetLastError();
}

} // namespace pixo_dev
