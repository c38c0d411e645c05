// png_reduce.hip — the PNG reductions on the device (gfx950): what the reference does to the pixels before it filters them
// (src/png/mod.rs:522-554): maybe_reduce_color_type (palette, colour type, bit depth) and maybe_optimize_alpha.
//
//   analyse        one read pass: all opaque? all gray (and the gray maximum)? a pixel with alpha 0? the set of distinct colour
//                  keys up to 256.  Every workgroup collects keys in an LDS hash set and merges it into a small global one
//                  when it is done; a flag says "more than 256", and a pass that has nothing left to learn leaves.
//   index          pixel -> index into the sorted keys (the host sorted them; lookup through an LDS copy of a hash table),
//                  histogram of the indices (per-thread runs, LDS counters, one global add per bin and workgroup)
//   cooccurrence   adjacent pairs of different indices, counted once at [min][max].  n <= 64: the n x n counters are
//                  private to the workgroup in LDS (16 KiB) and added to the global ones at the end; above that
//                  (n * n u32 does not fit) the adds go to global memory directly — pairs of equal indices, the
//                  hot cells of a smooth image, are not counted at all because the ordering never reads the diagonal.
//   convert        every byte of a reduced row is a pure function of (row, byte) — png_reduce_math.h reduced_byte; a
//                  thread makes four of them and stores one dword.
// Every kernel walks its work with a grid-stride loop bounded by the element count; nothing is read or written
// outside [0, pixels * spp) of the source and the documented sizes of the outputs.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "png_reduce.hpp"

namespace pixo_dev {
using namespace pixo_pngr;

namespace {
constexpr int kThreads = 256;
constexpr uint64_t kMaxBlocks = 2048; // memory-bound passes: 8 workgroups per CU, the rest by grid stride

__device__ __forceinline__ uint32_t peek(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The 4 pixels of group g (pixels 4g .. 4g + 3) as SPP dwords; pixels past the end read as 0.
template <int SPP>
__device__ __forceinline__ uint32_t load_group(const uint8_t *src, uint64_t g, uint64_t npix, bool aligned, uint32_t (&w)[SPP])
{
    const uint64_t first = 4 * g;
    const uint32_t valid = npix - first >= 4 ? 4u : (uint32_t)(npix - first);
    if (aligned && valid == 4) {
        if constexpr (SPP == 4) {
            const uint4 v = reinterpret_cast<const uint4 *>(src)[g];
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else if constexpr (SPP == 2) {
            const uint2 v = reinterpret_cast<const uint2 *>(src)[g];
            w[0] = v.x; w[1] = v.y;
        } else {
#pragma unroll
            for (int d = 0; d < SPP; ++d) w[d] = reinterpret_cast<const uint32_t *>(src)[g * SPP + d];
        }
    } else {
#pragma unroll
        for (int d = 0; d < SPP; ++d) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t byte = 4 * d + k;
                if (byte / SPP < valid) v |= (uint32_t)src[first * SPP + byte] << (8 * k);
            }
            w[d] = v;
        }
    }
    return valid;
}
template <int SPP> __device__ __forceinline__ uint32_t group_byte(const uint32_t (&w)[SPP], uint32_t byte)
{
    return (w[byte >> 2] >> (8 * (byte & 3))) & 0xFFu;
}

// 0: the key was there, 1: inserted, 2: no free slot (more than 256 keys anyway).  Slots only ever go from 0 to their
// final value, so a stale read of 0 is repaired by the compare-and-swap.
__device__ __forceinline__ int set_insert(unsigned long long *set, uint32_t key)
{
    const unsigned long long slot = kSlotUsed | key;
    uint32_t s = key_hash(key);
    for (uint32_t probes = 0; probes < kSetSlots; ++probes, s = (s + 1) & (kSetSlots - 1)) {
        unsigned long long e = *reinterpret_cast<volatile unsigned long long *>(set + s);
        if (e == slot) return 0;
        if (e == 0) {
            e = atomicCAS(set + s, 0ull, slot);
            if (e == 0) return 1;
            if (e == slot) return 0;
        }
    }
    return 2;
}

template <int SPP>
__global__ __launch_bounds__(kThreads) void png_analyse_kernel(const uint8_t *src, uint64_t npix, uint32_t want, bool aligned,
                                                               PngAnalysis *st)
{
    __shared__ unsigned long long set[kSetSlots];
    __shared__ uint32_t l_count, l_flags, l_max;
    const uint32_t tid = threadIdx.x;
    for (uint32_t s = tid; s < kSetSlots; s += kThreads) set[s] = 0;
    if (tid == 0) { l_count = 0; l_flags = 0; l_max = 0; }
    __syncthreads();

    uint32_t flags = 0, gmax = 0, prev_key = 0;
    bool have_prev = false;
    const uint64_t groups = (npix + 3) / 4;
    for (uint64_t g = (uint64_t)blockIdx.x * kThreads + tid; g < groups; g += (uint64_t)gridDim.x * kThreads) {
        const uint32_t seen = peek(&st->flags) | flags | *reinterpret_cast<volatile uint32_t *>(&l_flags);
        if ((seen & want) == want) break; // every question has its answer
        uint32_t w[SPP];
        const uint32_t valid = load_group<SPP>(src, g, npix, aligned, w);
        for (uint32_t p = 0; p < valid; ++p) {
            if constexpr (SPP == 2) {
                if (group_byte<SPP>(w, 2 * p + 1) == 0) flags |= PNG_A_ALPHA0;
            } else {
                const uint32_t r = group_byte<SPP>(w, SPP * p), gr = group_byte<SPP>(w, SPP * p + 1), b = group_byte<SPP>(w, SPP * p + 2);
                const uint32_t a = SPP == 4 ? group_byte<SPP>(w, SPP * p + 3) : 255u;
                if (a != 255) flags |= PNG_A_NON_OPAQUE;
                if (a == 0) flags |= PNG_A_ALPHA0;
                if (r != gr || gr != b) flags |= PNG_A_NON_GRAY;
                gmax = max(gmax, r);
                if ((want & PNG_A_OVERFLOW) && !(seen & PNG_A_OVERFLOW) && !(flags & PNG_A_OVERFLOW)) {
                    const uint32_t key = (r << 24) | (gr << 16) | (b << 8) | a;
                    if (!have_prev || key != prev_key) {
                        const int res = set_insert(set, key);
                        if (res == 2 || (res == 1 && atomicAdd(&l_count, 1u) + 1 > 256)) {
                            flags |= PNG_A_OVERFLOW; // the workgroup's first thread to notice tells the other workgroups
                            if (!(atomicOr(&l_flags, (uint32_t)PNG_A_OVERFLOW) & PNG_A_OVERFLOW)) atomicOr(&st->flags, (uint32_t)PNG_A_OVERFLOW);
                        }
                        prev_key = key;
                        have_prev = true;
                    }
                }
            }
        }
    }
    if (flags) atomicOr(&l_flags, flags);
    if (gmax) atomicMax(&l_max, gmax);
    __syncthreads();
    const uint32_t wg_flags = l_flags;
    if (tid == 0) {
        if (wg_flags & ~peek(&st->flags)) atomicOr(&st->flags, wg_flags);
        if (l_max) atomicMax(&st->gray_max, l_max);
    }
    if (!(want & PNG_A_OVERFLOW) || (wg_flags & PNG_A_OVERFLOW)) return;
    unsigned long long *table = reinterpret_cast<unsigned long long *>(st->table);
    for (uint32_t s = tid; s < kSetSlots; s += kThreads) {
        const unsigned long long e = set[s];
        if (!e) continue;
        if (peek(&st->flags) & PNG_A_OVERFLOW) break;
        const int res = set_insert(table, (uint32_t)e);
        if (res == 2 || (res == 1 && atomicAdd(&st->count, 1u) + 1 > 256)) atomicOr(&st->flags, (uint32_t)PNG_A_OVERFLOW);
    }
}

template <int SPP>
__global__ __launch_bounds__(kThreads) void png_index_kernel(const uint8_t *src, uint64_t npix, bool aligned, const uint64_t *lookup,
                                                             uint8_t *index, uint32_t *hist)
{
    __shared__ uint64_t table[kSetSlots];
    __shared__ uint32_t l_hist[256];
    const uint32_t tid = threadIdx.x;
    for (uint32_t s = tid; s < kSetSlots; s += kThreads) table[s] = lookup[s];
    l_hist[tid] = 0; // (kThreads == 256)
    __syncthreads();
    uint32_t prev_key = 0, run_index = 0, run = 0; // run: pixels of run_index not yet in the histogram
    bool have_prev = false;
    const uint64_t groups = (npix + 3) / 4;
    for (uint64_t g = (uint64_t)blockIdx.x * kThreads + tid; g < groups; g += (uint64_t)gridDim.x * kThreads) {
        uint32_t w[SPP];
        const uint32_t valid = load_group<SPP>(src, g, npix, aligned, w);
        uint32_t out = 0;
        for (uint32_t p = 0; p < valid; ++p) {
            const uint32_t r = group_byte<SPP>(w, SPP * p), gr = group_byte<SPP>(w, SPP * p + 1), b = group_byte<SPP>(w, SPP * p + 2);
            const uint32_t a = SPP == 4 ? group_byte<SPP>(w, SPP * p + 3) : 255u;
            const uint32_t key = (r << 24) | (gr << 16) | (b << 8) | a;
            if (!have_prev || key != prev_key) {
                if (run) atomicAdd(&l_hist[run_index], run);
                run = 0;
                run_index = lookup_index(table, key);
                prev_key = key;
                have_prev = true;
            }
            ++run;
            out |= run_index << (8 * p);
        }
        if (valid == 4) reinterpret_cast<uint32_t *>(index)[g] = out;
        else for (uint32_t p = 0; p < valid; ++p) index[4 * g + p] = (uint8_t)(out >> (8 * p));
    }
    if (run) atomicAdd(&l_hist[run_index], run);
    __syncthreads();
    if (l_hist[tid]) atomicAdd(&hist[tid], l_hist[tid]);
}

// PRIVATE: the n * n counters live in LDS (n <= 64)
template <bool PRIVATE>
__global__ __launch_bounds__(kThreads) void png_cooccurrence_kernel(const uint8_t *index, uint32_t width, uint32_t height, uint32_t n,
                                                                    uint32_t *pairs)
{
    __shared__ uint32_t l_pairs[PRIVATE ? 64 * 64 : 1];
    const uint32_t tid = threadIdx.x;
    if (PRIVATE) {
        for (uint32_t s = tid; s < n * n; s += kThreads) l_pairs[s] = 0;
        __syncthreads();
    }
    uint32_t *counters = PRIVATE ? l_pairs : pairs;
    const uint64_t npix = (uint64_t)width * height;
    for (uint64_t p = (uint64_t)blockIdx.x * kThreads + tid; p < npix; p += (uint64_t)gridDim.x * kThreads) {
        const uint32_t x = (uint32_t)(p % width);
        const uint32_t v = index[p];
        if (x + 1 < width) {
            const uint32_t o = index[p + 1];
            if (o != v && v < n && o < n) atomicAdd(&counters[min(v, o) * n + max(v, o)], 1u);
        }
        if (p + width < npix) {
            const uint32_t o = index[p + width];
            if (o != v && v < n && o < n) atomicAdd(&counters[min(v, o) * n + max(v, o)], 1u);
        }
    }
    if (PRIVATE) {
        __syncthreads();
        for (uint32_t s = tid; s < n * n; s += kThreads)
            if (l_pairs[s]) atomicAdd(&pairs[s], l_pairs[s]);
    }
}

__global__ __launch_bounds__(kThreads) void png_convert_kernel(ConvertArgs a, const uint8_t *src, const uint8_t *map, uint8_t *dst)
{
    __shared__ uint8_t l_map[256];
    if (a.form == FORM_INDEX) {
        l_map[threadIdx.x] = map[threadIdx.x]; // (kThreads == 256)
        __syncthreads();
    }
    const uint64_t total = (uint64_t)a.row_bytes * a.height, dwords = (total + 3) / 4;
    for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < dwords; t += (uint64_t)gridDim.x * kThreads) {
        uint32_t y = (uint32_t)(4 * t / a.row_bytes), j = (uint32_t)(4 * t % a.row_bytes);
        uint32_t out = 0;
        for (uint32_t k = 0; k < 4 && 4 * t + k < total; ++k) {
            out |= (uint32_t)reduced_byte(a, src, l_map, y, j) << (8 * k);
            if (++j == a.row_bytes) { j = 0; ++y; }
        }
        reinterpret_cast<uint32_t *>(dst)[t] = out; // (the destination is rounded up to whole dwords)
    }
}

uint32_t blocks_for(uint64_t items)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kMaxBlocks, (items + kThreads - 1) / kThreads));
}
bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
} // namespace

hipError_t launch_png_analyse(const void *d_pixels, uint64_t pixels, uint32_t spp, uint32_t want, PngAnalysis *d_state,
                              hipStream_t stream)
{
    static_assert(sizeof(PngAnalysis) % 16 == 0, "zeroed with one memset");
    hipError_t e = hipMemsetAsync(d_state, 0, sizeof(PngAnalysis), stream);
    if (e != hipSuccess || pixels == 0) return e;
    const uint8_t *src = static_cast<const uint8_t *>(d_pixels);
    const uint32_t blocks = blocks_for((pixels + 3) / 4);
    const bool al = aligned16(d_pixels);
    switch (spp) {
    case 2: png_analyse_kernel<2><<<blocks, kThreads, 0, stream>>>(src, pixels, want & PNG_A_ALPHA0, al, d_state); break;
    case 3: png_analyse_kernel<3><<<blocks, kThreads, 0, stream>>>(src, pixels, want & (PNG_A_OVERFLOW | PNG_A_NON_GRAY), al, d_state); break;
    case 4: png_analyse_kernel<4><<<blocks, kThreads, 0, stream>>>(src, pixels, want, al, d_state); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_png_index(const void *d_pixels, uint64_t pixels, uint32_t spp, const uint64_t *d_lookup, uint8_t *d_index,
                            uint32_t *d_hist, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(d_hist, 0, 256 * sizeof(uint32_t), stream);
    if (e != hipSuccess || pixels == 0) return e;
    const uint8_t *src = static_cast<const uint8_t *>(d_pixels);
    const uint32_t blocks = blocks_for((pixels + 3) / 4);
    const bool al = aligned16(d_pixels);
    if (spp == 3) png_index_kernel<3><<<blocks, kThreads, 0, stream>>>(src, pixels, al, d_lookup, d_index, d_hist);
    else if (spp == 4) png_index_kernel<4><<<blocks, kThreads, 0, stream>>>(src, pixels, al, d_lookup, d_index, d_hist);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_png_cooccurrence(const uint8_t *d_index, uint32_t width, uint32_t height, uint32_t n, uint32_t *d_pairs,
                                   hipStream_t stream)
{
    if (n == 0 || n > 256) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_pairs, 0, (size_t)n * n * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint32_t blocks = blocks_for((uint64_t)width * height);
    if (n <= 64) png_cooccurrence_kernel<true><<<blocks, kThreads, 0, stream>>>(d_index, width, height, n, d_pairs);
    else png_cooccurrence_kernel<false><<<blocks, kThreads, 0, stream>>>(d_index, width, height, n, d_pairs);
    return hipGetLastError();
}

hipError_t launch_png_convert(const ConvertArgs &a, const void *d_src, const uint8_t *d_map, void *d_dst, hipStream_t stream)
{
    if (a.row_bytes == 0 || a.height == 0) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)a.row_bytes * a.height;
    png_convert_kernel<<<blocks_for((total + 3) / 4), kThreads, 0, stream>>>(a, static_cast<const uint8_t *>(d_src), d_map,
                                                                            static_cast<uint8_t *>(d_dst));
    return hipGetLastError();
}

} // namespace pixo_dev
