// png_unfilter.hip — the device stage of the PNG decoder (gfx950): what reconstruct_image and convert_to_pixels
// (src/decode/png.rs:294-533) do to every byte.  The arithmetic is png_unfilter_math.h.
//
//   unfilter  Row reconstruction on the skewed wavefront.  A reconstructed byte needs its left, above and above-left
//             neighbours.  Row 0 and every row filtered None or Sub do not read the row above: they cut the image into
//             runs that are independent of each other.  A workgroup (one wavefront) owns a run and walks it with a row per
//             lane, 64 rows a pass.  A lane reads and writes its row in 16-byte pieces and lags the lane above by one
//             piece: at step s lane l is at piece s - l, the piece above it was finished one step earlier by lane l - 1 and
//             arrives by four lane shuffles, the above-left bytes are the tail of the piece that arrived the step before,
//             the left bytes are the tail of the lane's own last piece — all in registers.  (The lag is a piece and not a
//             pixel because 16 is no multiple of the 3- and 6-byte filter units; inside a piece every index is a constant.)
//             The filter is a per-lane select, not a branch: a wavefront of mixed rows runs one instruction stream.
//             A run longer than 64 rows is walked in passes; the last row of a pass is in global memory, fenced, before the
//             first lane of the next pass reads it.  No workgroup waits for another anywhere: the launch finishes whatever
//             the dispatch order.  An image of one run (every row Paeth) runs on one wavefront.
//   convert   Element-wise: 8-bit rows copy through, 16-bit samples keep their high byte, packed gray is unpacked and
//             scaled, palette indices go through a 256-word table in LDS.
// Bounds: unfilter reads stream bytes below unfilter_stream_alloc(height, row_bytes) (piece indices are clamped into the
// row), writes rows[r * pitch + 16 k] for r < height, 16 k < pitch; convert reads rows below height * pitch and writes
// out below width * height * out_bpp.
//   batches   The same two stages over the images of a sub-batch: one unfilter launch per filter unit (the unit stays a
//             compile-time constant), a workgroup per run of any image, and one convert launch per kernel form, a workgroup
//             serving one image.  A workgroup reads its run record and its image's description (UnfilterBatchImage) — the
//             same for all its lanes, scalar loads — and then runs the single kernels' bodies on that image's addresses.
//             Still no workgroup waits for another.
// Bounds of the batch forms: image i's stream lies at stream + stream_at, height * (row_bytes + 1) bytes, the streams one
// behind the other; piece indices are clamped into their row, so unfilter reads at most 15 bytes past an image's last row,
// which is the next image's stream or, behind the last one, the 16 bytes the buffer has to spare.  It writes
// rows + rows_at + r * pitch + 16 k for r < height, 16 k < pitch: the image's own height * pitch bytes (rows_at is a multiple
// of 16, the images' rows do not overlap).  convert reads those bytes and writes out + out_at below width * height * out_bpp
// — never the bytes between two images — with 16-byte and dword stores only where the caller found the REAL address
// out + out_at aligned (kernel form, aligned4); a palette image reads the 256 words at tables + table_at.  A run record's
// image is below the batch's size, a block table's entry too (the host wrote both).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "png_unfilter.hpp"

namespace pixo_dev {
using namespace pixo_pngu;

namespace {
constexpr int kThreads = 256;
constexpr uint64_t kMaxBlocks = 1u << 16;

uint32_t blocks_for(uint64_t items) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kMaxBlocks, (items + kThreads - 1) / kThreads)); }

struct Piece {
    uint32_t w[4];
};
__device__ __forceinline__ uint32_t byte_of(const Piece &p, int j) { return (p.w[j >> 2] >> (8 * (j & 3))) & 255u; }
__device__ __forceinline__ Piece load_piece(const uint8_t *p) // any alignment
{
    Piece v;
    __builtin_memcpy(&v, p, sizeof v);
    return v;
}
__device__ __forceinline__ Piece shuffle_up(const Piece &p)
{
    Piece v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v.w[i] = (uint32_t)__shfl_up((int)p.w[i], 1);
    return v;
}

// One piece of a row: `in` filtered, `left` the lane's piece before it, `up` the piece above, `up_left` the piece above `left`.
// HEAVY false: no row of the pass is Average or Paeth.
template <int BPP, bool HEAVY> __device__ __forceinline__ Piece reconstruct_piece(uint32_t filter, const Piece &in, const Piece &left, const Piece &up, const Piece &up_left)
{
    uint32_t o[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t a = j >= BPP ? o[j >= BPP ? j - BPP : 0] : byte_of(left, 16 - BPP + j);
        const uint32_t b = byte_of(up, j);
        if (HEAVY) {
            const uint32_t c = j >= BPP ? byte_of(up, j >= BPP ? j - BPP : 0) : byte_of(up_left, 16 - BPP + j);
            o[j] = reconstruct(filter, byte_of(in, j), a, b, c);
        } else
            o[j] = (byte_of(in, j) + (filter == FILTER_SUB ? a : filter == FILTER_UP ? b : 0u)) & 255u;
    }
    Piece r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.w[i] = o[4 * i] | (o[4 * i + 1] << 8) | (o[4 * i + 2] << 16) | (o[4 * i + 3] << 24);
    return r;
}

// One run of rows on the calling wavefront: rows run_row .. run_row + run_rows - 1 of the image whose stream and rows these are
template <int BPP> __device__ __forceinline__ void unfilter_run(const UnfilterArgs &a, uint32_t run_row, uint32_t run_rows)
{
    static_assert(kUnfilterPassRows == 64 && kUnfilterPiece == 16, "a row per lane of one wavefront, 16-byte pieces");
    const uint32_t lane = threadIdx.x;
    const int64_t pieces = (int64_t)(a.pitch / kUnfilterPiece);
    const Piece zero = {{0, 0, 0, 0}};
    for (uint32_t base = 0; base < run_rows; base += kUnfilterPassRows) {
        const uint32_t rows = min(kUnfilterPassRows, run_rows - base);
        const bool active = lane < rows;
        const uint64_t r = (uint64_t)run_row + base + (active ? lane : 0u);
        const uint8_t *src = a.stream + r * (a.row_bytes + 1);
        const uint32_t filter = src[0];
        ++src;
        uint8_t *dst = a.rows + r * a.pitch;
        // The pass's first lane takes the row above from memory: the last row of the pass before (none above a run's first row,
        // which does not read it; above row 0 the reference has zeros).
        const bool from_memory = lane == 0 && base > 0;
        const uint8_t *above = from_memory ? dst - a.pitch : a.rows;
        const bool heavy = __any(active && filter >= FILTER_AVERAGE);

        Piece left = zero, up_left = zero, made = zero;
        int64_t k = -(int64_t)lane;
        // What a step needs from memory is asked for one step ahead (piece indices clamped into the row: always in bounds).
        Piece in_next = load_piece(src), above_next = from_memory ? load_piece(above) : zero;
        const int64_t steps = pieces + rows - 1;
        for (int64_t s = 0; s < steps; ++s, ++k) {
            Piece up = shuffle_up(made);
            const Piece in = in_next;
            if (lane == 0) up = above_next;
            const int64_t k1 = min(max(k + 1, (int64_t)0), pieces - 1);
            in_next = load_piece(src + k1 * kUnfilterPiece);
            if (from_memory) above_next = load_piece(above + k1 * kUnfilterPiece);
            if (active && k >= 0 && k < pieces) {
                made = heavy ? reconstruct_piece<BPP, true>(filter, in, left, up, up_left) : reconstruct_piece<BPP, false>(filter, in, left, up, up_left);
                *reinterpret_cast<uint4 *>(dst + k * kUnfilterPiece) = make_uint4(made.w[0], made.w[1], made.w[2], made.w[3]);
                left = made;
                up_left = up;
            }
        }
        __threadfence(); // the pass's last row is in memory before the next pass's first lane reads it
        __syncthreads();
    }
}

template <int BPP> __global__ __launch_bounds__(kUnfilterPassRows) void png_unfilter_kernel(const UnfilterArgs a)
{
    unfilter_run<BPP>(a, a.runs[2 * blockIdx.x], a.runs[2 * blockIdx.x + 1]);
}

// The batch form: workgroup blockIdx.x reads its run record and its image's description — both the same for every lane, so
// the loads are scalar — and walks the run as the single kernel does.
template <int BPP> __global__ __launch_bounds__(kUnfilterPassRows) void png_unfilter_batch_kernel(const UnfilterBatchArgs b)
{
    const UnfilterBatchRun run = b.runs[blockIdx.x];
    const UnfilterBatchImage &im = b.images[run.image];
    UnfilterArgs a;
    a.stream = b.stream + im.stream_at;
    a.rows = b.rows + im.rows_at;
    a.row_bytes = im.row_bytes;
    a.pitch = im.pitch;
    a.bpp = BPP;
    a.runs = nullptr;
    a.n_runs = 0;
    unfilter_run<BPP>(a, run.first_row, run.rows);
}

// The conversion's three bodies: thread `first` of `step` of one image's launch share (the single kernels: of the grid).
// 8-bit rows, 16 output bytes a thread: rows of a multiple of 16 bytes into 16-byte aligned storage
__device__ __forceinline__ void convert_copy16(const UnconvertArgs &a, uint64_t row_out, uint64_t first, uint64_t step)
{
    const uint64_t per_row = row_out / 16, total = per_row * a.height;
    for (uint64_t g = first; g < total; g += step) {
        const uint64_t y = g / per_row, i = (g - y * per_row) * 16;
        *reinterpret_cast<uint4 *>(a.out + y * row_out + i) = *reinterpret_cast<const uint4 *>(a.rows + y * a.pitch + i);
    }
}
// The byte-wise forms (copy, high byte), four output bytes a thread
__device__ __forceinline__ void convert_bytes(const UnconvertArgs &a, uint64_t row_out, bool aligned4, uint64_t first_group, uint64_t step)
{
    const uint64_t total = row_out * a.height, groups = (total + 3) / 4;
    for (uint64_t g = first_group; g < groups; g += step) {
        const uint64_t first = 4 * g;
        const uint32_t valid = total - first >= 4 ? 4u : (uint32_t)(total - first);
        uint64_t y = first / row_out, i = first - y * row_out;
        uint32_t word = 0;
        for (uint32_t k = 0; k < valid; ++k) {
            word |= convert_byte(a.form, a.rows + y * a.pitch, i) << (8 * k);
            if (++i == row_out) { i = 0; ++y; }
        }
        if (valid == 4 && aligned4) reinterpret_cast<uint32_t *>(a.out)[g] = word;
        else
            for (uint32_t k = 0; k < valid; ++k) a.out[first + k] = (uint8_t)(word >> (8 * k));
    }
}
// The sample-wise forms (packed gray, palette), a pixel a thread; `table`: the image's palette in LDS
__device__ __forceinline__ void convert_samples(const UnconvertArgs &a, bool aligned4, const uint32_t *table, uint64_t first, uint64_t step)
{
    const uint64_t pixels = (uint64_t)a.width * a.height;
    for (uint64_t p = first; p < pixels; p += step) {
        const uint64_t y = p / a.width, x = p - y * a.width;
        const uint32_t v = convert_sample(a.form, a.rows + y * a.pitch, x, a.depth, table);
        if (a.out_bpp == 4 && aligned4) reinterpret_cast<uint32_t *>(a.out)[p] = v;
        else
            for (uint32_t k = 0; k < a.out_bpp; ++k) a.out[p * a.out_bpp + k] = (uint8_t)(v >> (8 * k));
    }
}

__global__ __launch_bounds__(kThreads) void png_convert_copy16_kernel(const UnconvertArgs a, uint64_t row_out)
{
    convert_copy16(a, row_out, (uint64_t)blockIdx.x * kThreads + threadIdx.x, (uint64_t)gridDim.x * kThreads);
}
__global__ __launch_bounds__(kThreads) void png_convert_bytes_kernel(const UnconvertArgs a, uint64_t row_out, bool aligned4)
{
    convert_bytes(a, row_out, aligned4, (uint64_t)blockIdx.x * kThreads + threadIdx.x, (uint64_t)gridDim.x * kThreads);
}
__global__ __launch_bounds__(kThreads) void png_convert_samples_kernel(const UnconvertArgs a, bool aligned4)
{
    __shared__ uint32_t table[256];
    if (a.form == CONVERT_PALETTE) table[threadIdx.x] = a.table[threadIdx.x]; // (kThreads == 256)
    __syncthreads();
    convert_samples(a, aligned4, table, (uint64_t)blockIdx.x * kThreads + threadIdx.x, (uint64_t)gridDim.x * kThreads);
}

// The batch forms: the workgroups of row blockIdx.y of the grid serve image list[blockIdx.y] — one image a workgroup, its
// palette in LDS — and stride over it by gridDim.x workgroups (a grid sized for the list's largest image: a workgroup beyond
// a smaller image's work finds its loop empty).
__device__ __forceinline__ UnconvertArgs batch_image(const UnconvertBatchArgs &b, const UnfilterBatchImage &im)
{
    UnconvertArgs a;
    a.rows = b.rows + im.rows_at; a.pitch = im.pitch; a.out = b.out + im.out_at; a.width = im.width; a.height = im.height;
    a.form = im.form; a.depth = im.depth; a.out_bpp = im.out_bpp; a.table = b.tables + im.table_at;
    return a;
}
__global__ __launch_bounds__(kThreads) void png_convert_copy16_batch_kernel(const UnconvertBatchArgs b)
{
    const UnfilterBatchImage &im = b.images[b.list[blockIdx.y]];
    convert_copy16(batch_image(b, im), (uint64_t)im.width * im.out_bpp, (uint64_t)blockIdx.x * kThreads + threadIdx.x, (uint64_t)gridDim.x * kThreads);
}
__global__ __launch_bounds__(kThreads) void png_convert_bytes_batch_kernel(const UnconvertBatchArgs b)
{
    const UnfilterBatchImage &im = b.images[b.list[blockIdx.y]];
    convert_bytes(batch_image(b, im), (uint64_t)im.width * im.out_bpp, im.aligned4 != 0, (uint64_t)blockIdx.x * kThreads + threadIdx.x,
                  (uint64_t)gridDim.x * kThreads);
}
__global__ __launch_bounds__(kThreads) void png_convert_samples_batch_kernel(const UnconvertBatchArgs b)
{
    __shared__ uint32_t table[256];
    const UnfilterBatchImage &im = b.images[b.list[blockIdx.y]];
    const UnconvertArgs a = batch_image(b, im);
    if (a.form == CONVERT_PALETTE) table[threadIdx.x] = a.table[threadIdx.x]; // (kThreads == 256)
    __syncthreads();
    convert_samples(a, im.aligned4 != 0, table, (uint64_t)blockIdx.x * kThreads + threadIdx.x, (uint64_t)gridDim.x * kThreads);
}
static_assert(kThreads == 256, "the palette table is loaded a word a thread");

} // namespace

hipError_t launch_png_unfilter(const UnfilterArgs &a, hipStream_t stream)
{
    if (!a.stream || !a.rows || !a.runs || !a.n_runs || !a.row_bytes || a.pitch != unfilter_pitch(a.row_bytes) ||
        reinterpret_cast<uintptr_t>(a.rows) % 16)
        return hipErrorInvalidValue;
    switch (a.bpp) {
    case 1: png_unfilter_kernel<1><<<a.n_runs, kUnfilterPassRows, 0, stream>>>(a); break;
    case 2: png_unfilter_kernel<2><<<a.n_runs, kUnfilterPassRows, 0, stream>>>(a); break;
    case 3: png_unfilter_kernel<3><<<a.n_runs, kUnfilterPassRows, 0, stream>>>(a); break;
    case 4: png_unfilter_kernel<4><<<a.n_runs, kUnfilterPassRows, 0, stream>>>(a); break;
    case 6: png_unfilter_kernel<6><<<a.n_runs, kUnfilterPassRows, 0, stream>>>(a); break;
    case 8: png_unfilter_kernel<8><<<a.n_runs, kUnfilterPassRows, 0, stream>>>(a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_png_convert(const UnconvertArgs &a, hipStream_t stream)
{
    if (!a.rows || !a.out || !a.width || !a.height || a.form > CONVERT_PALETTE || !a.out_bpp || a.out_bpp > 4) return hipErrorInvalidValue;
    const bool aligned4 = reinterpret_cast<uintptr_t>(a.out) % 4 == 0;
    if (a.form == CONVERT_COPY || a.form == CONVERT_HIGH) {
        const uint64_t row_out = (uint64_t)a.width * a.out_bpp;
        if (a.form == CONVERT_COPY && row_out % 16 == 0 && reinterpret_cast<uintptr_t>(a.out) % 16 == 0)
            png_convert_copy16_kernel<<<blocks_for(row_out / 16 * a.height), kThreads, 0, stream>>>(a, row_out);
        else
            png_convert_bytes_kernel<<<blocks_for((row_out * a.height + 3) / 4), kThreads, 0, stream>>>(a, row_out, aligned4);
    } else {
        if (a.form == CONVERT_PALETTE && !a.table) return hipErrorInvalidValue;
        if (a.depth != 1 && a.depth != 2 && a.depth != 4 && a.depth != 8) return hipErrorInvalidValue;
        png_convert_samples_kernel<<<blocks_for((uint64_t)a.width * a.height), kThreads, 0, stream>>>(a, aligned4);
    }
    return hipGetLastError();
}

hipError_t launch_png_unfilter_batch(const UnfilterBatchArgs &a, hipStream_t stream)
{
    if (!a.stream || !a.rows || !a.images || !a.runs || !a.n_runs || reinterpret_cast<uintptr_t>(a.rows) % 16 ||
        reinterpret_cast<uintptr_t>(a.images) % 16 || reinterpret_cast<uintptr_t>(a.runs) % 16)
        return hipErrorInvalidValue;
    switch (a.bpp) {
    case 1: png_unfilter_batch_kernel<1><<<a.n_runs, kUnfilterPassRows, 0, stream>>>(a); break;
    case 2: png_unfilter_batch_kernel<2><<<a.n_runs, kUnfilterPassRows, 0, stream>>>(a); break;
    case 3: png_unfilter_batch_kernel<3><<<a.n_runs, kUnfilterPassRows, 0, stream>>>(a); break;
    case 4: png_unfilter_batch_kernel<4><<<a.n_runs, kUnfilterPassRows, 0, stream>>>(a); break;
    case 6: png_unfilter_batch_kernel<6><<<a.n_runs, kUnfilterPassRows, 0, stream>>>(a); break;
    case 8: png_unfilter_batch_kernel<8><<<a.n_runs, kUnfilterPassRows, 0, stream>>>(a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_png_convert_batch(const UnconvertBatchArgs &a, hipStream_t stream)
{
    if (!a.rows || !a.out || !a.images || !a.list || !a.n || a.n > 65535 || !a.tables || !a.max_items || a.kernel >= CONVERT_KERNELS)
        return hipErrorInvalidValue;
    // the grid's rows are the images; its width serves the largest of them, within about 2^20 workgroups in all
    const uint32_t wide = std::max<uint32_t>(256, (1u << 20) / a.n);
    const dim3 grid(std::min(blocks_for(a.max_items), wide), a.n);
    if (a.kernel == CONVERT_KERNEL_COPY16) png_convert_copy16_batch_kernel<<<grid, kThreads, 0, stream>>>(a);
    else if (a.kernel == CONVERT_KERNEL_BYTES) png_convert_bytes_batch_kernel<<<grid, kThreads, 0, stream>>>(a);
    else png_convert_samples_batch_kernel<<<grid, kThreads, 0, stream>>>(a);
    return hipGetLastError();
}

} // namespace pixo_dev
