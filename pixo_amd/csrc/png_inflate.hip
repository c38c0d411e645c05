// png_inflate.hip — inflate on the device for the PNG decode batches (gfx950).  DEFLATE is sequential inside a stream, a
// batch holds N independent streams: one launch inflates all streams of a sub-batch, a workgroup of ONE wavefront per stream.
// The walk — bit buffer, tables, tokens, the LDS ring, the flush with its Adler-32 — is png_inflate_math.h, the same text the
// host build of tests/emu_png_inflate/ runs lane by lane.
//
// No workgroup waits for another: no flags, no look-back, no spinning; the launch finishes whatever the dispatch order.  A
// stream's workgroup reads only its own padded input (aligned dword loads below 4 * ceil(in_len / 4), byte loads of stored
// blocks below in_len) and writes only [out_at, out_at + expected) and its own status record; matches read the LDS ring,
// never global memory this launch wrote.  Everything leaves the kernel through vector stores.
//
//   gather  The filter byte of every row of every image into one compact array, so that the host can cut the runs of rows
//           without the inflated streams ever coming down.  A launch of its own behind the inflate: what it reads was
//           written by the launch before it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "png_inflate_dev.hpp"

namespace pixo_dev {

namespace {
constexpr int kGatherThreads = 256;

__global__ __launch_bounds__(pixo_pngi::kLanes) void png_inflate_kernel(const uint8_t *__restrict__ input, uint8_t *__restrict__ out,
                                                                        const InflateStream *__restrict__ streams, InflateStatus *__restrict__ status)
{
    __shared__ pixo_pngi::Shared sh;
    const InflateStream d = streams[blockIdx.x];
    pixo_pngi::Walk walk(sh, input + d.in_at, d.in_len, out + d.out_at, d.expected);
    const pixo_pngi::Result r = walk.run();
    if (threadIdx.x == 0) {
        InflateStatus s;
        s.verdict = r.verdict; s.adler = r.adler; s.produced = r.produced;
        status[blockIdx.x] = s;
    }
}

// Row blockIdx.y of the grid serves image blockIdx.y and strides over its rows
__global__ __launch_bounds__(kGatherThreads) void png_filter_gather_kernel(const FilterGatherArgs a)
{
    const FilterGatherImage im = a.images[blockIdx.y];
    for (uint32_t y = blockIdx.x * kGatherThreads + threadIdx.x; y < im.height; y += gridDim.x * kGatherThreads)
        a.filters[im.filters_at + y] = a.stream[im.stream_at + (uint64_t)y * im.stride];
}
} // namespace

hipError_t launch_png_inflate(const InflateArgs &a, hipStream_t stream)
{
    if (!a.input || !a.out || !a.streams || !a.status || !a.n || a.n > 65535 || reinterpret_cast<uintptr_t>(a.input) % kInflateInputAlign ||
        reinterpret_cast<uintptr_t>(a.streams) % 16 || reinterpret_cast<uintptr_t>(a.status) % 16)
        return hipErrorInvalidValue;
    png_inflate_kernel<<<a.n, pixo_pngi::kLanes, 0, stream>>>(a.input, a.out, a.streams, a.status);
    return hipGetLastError();
}

hipError_t launch_png_filter_gather(const FilterGatherArgs &a, hipStream_t stream)
{
    if (!a.stream || !a.filters || !a.images || !a.n || a.n > 65535 || !a.max_height || reinterpret_cast<uintptr_t>(a.images) % 16)
        return hipErrorInvalidValue;
    const dim3 grid(std::min<uint32_t>(64, (a.max_height + kGatherThreads - 1) / kGatherThreads), a.n);
    png_filter_gather_kernel<<<grid, kGatherThreads, 0, stream>>>(a);
    return hipGetLastError();
}

} // namespace pixo_dev
