// jpeg_entropy_dec.hip — the Huffman decode of baseline scans on the device (PIXO_DECODE_DEVICE_ENTROPY): raw scans in HBM ->
// quantised coefficients in HBM, in the layout jpeg_decode.hip loads.  What a lane computes: jpeg_entropy_dec_math.h; here the
// scaffolding.  Four kernels, each one launch over all files of a sub-batch (a workgroup finds its file by the search over the
// records' first_group):
//   sync    a workgroup stages its 32 KiB of scan and its file's record (six Huffman tables) in LDS with 16-byte loads, decodes
//           its 256 subsequences cold (launch 0) or takes their states from HBM (later launches), and hands exit states from lane
//           to lane through LDS until nothing changes or the file's rounds are spent (status.used, written in turn like the borders).  Its first lane's predecessor is the last lane of
//           the workgroup in front AS OF THE PREVIOUS LAUNCH (two border arrays written in turn): no workgroup waits for another.
//           It counts itself in counters[2 * launch] when it must run again or its last exit changed.
//   verify  a workgroup per file: prefix sums of the block counts, the chain's checks, the file's status.
//   write   the sync kernel's grid: every lane of the verified chain decodes once more and stores ACs and DC differences.
//   dc      a workgroup per file and component: the wrap-around sum of the differences in scan order, truncated to int16.
#include <hip/hip_runtime.h>

#include "jpeg_decode_math.h"
#include "jpeg_entropy_dec.hpp"

namespace {

namespace je = pixo_jent;
static_assert(je::coef_index(12345, 37) == 192 * 4096 + 4 * 512 + 57 * 8 + 5, "the layout of jpeg_decode_math.h");
static_assert(je::kGroupSubs == 256, "a lane per subsequence");

__constant__ uint8_t kZigzagDev[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                       35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// The staged scan bytes of a workgroup (je::lds_at: padded against bank conflicts)
struct LdsBytes {
    const uint8_t *s;
    uint32_t lo;
    __device__ uint32_t operator()(uint32_t i) const { return s[je::lds_at(i - lo)]; }
};

// What sync and write share: the file's record and the workgroup's span of its scan into LDS
struct Staged {
    uint32_t file, group, lo, limit;
};
__device__ Staged stage(const je::FileRecord *records, uint32_t files, const uint8_t *scans, je::FileRecord *rec, uint32_t *bytes)
{
    Staged st;
    st.file = je::file_of_group(records, files, blockIdx.x);
    const je::FileRecord *mine = records + st.file;
    const uint4 *from = reinterpret_cast<const uint4 *>(mine);
    uint4 *to = reinterpret_cast<uint4 *>(rec);
    for (uint32_t i = threadIdx.x; i < sizeof(je::FileRecord) / 16; i += je::kGroupSubs) to[i] = from[i];
    st.group = blockIdx.x - mine->first_group;
    st.lo = je::stage_lo(st.group);
    const uint32_t hi = je::stage_hi(st.group, mine->ecs_len);
    st.limit = hi < mine->ecs_len ? hi : mine->ecs_len;
    const uint8_t *scan = scans + mine->ecs_at;
    for (uint32_t i = st.lo + threadIdx.x * 16; i < hi; i += je::kGroupSubs * 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(scan + i);
        uint32_t *at = bytes + je::lds_at(i - st.lo) / 4;
        at[0] = v.x; at[1] = v.y; at[2] = v.z; at[3] = v.w;
    }
    __syncthreads();
    return st;
}

__global__ __launch_bounds__(256) void jpeg_entropy_sync_kernel(pixo_dev::JpegEntropyArgs a, uint32_t launch, uint32_t cap)
{
    __shared__ __attribute__((aligned(16))) je::FileRecord rec;
    __shared__ __attribute__((aligned(16))) uint32_t bytes[je::kStageLds / 4];
    __shared__ je::State lexit[je::kGroupSubs];
    const Staged st = stage(a.records, a.files, a.scans, &rec, bytes);
    const LdsBytes by{reinterpret_cast<const uint8_t *>(bytes), st.lo};
    const uint32_t tid = threadIdx.x, j = st.group * je::kGroupSubs + tid, at = rec.first_sub + j;
    const bool active = j < rec.subs, cold = launch == 0;
    const je::State true_state = je::make_state(0, 0, 0);
    const je::State *border_in = a.border[launch & 1];
    je::State *border_out = a.border[(launch & 1) ^ 1];
    je::NoSink none;
    je::State entry = je::kDead, exit = je::kDead;
    uint32_t blocks = 0;
    if (active) {
        if (cold) {
            entry = j ? je::cold_entry(by, st.limit, j) : true_state;
            const je::Exit x = je::decode_sub(by, st.limit, rec, j, entry, ~0u, none);
            exit = x.state; blocks = x.packed();
        } else {
            entry = a.entry[at]; exit = a.exit[at]; blocks = a.count[at];
        }
    }
    lexit[tid] = exit;
    // what the file has used so far (the launch before wrote it; nobody writes it now) and what that leaves this launch
    const uint32_t used = a.status[st.file].used[launch & 1], budget = used < cap ? cap - used : 0u;
    uint32_t rounds = 0, unfinished = 0;
    for (;;) {
        __syncthreads(); // the exits of the turn before are in LDS
        je::State pred = true_state;
        bool need = false;
        if (active && !(cold && tid == 0 && st.group)) { // (launch 0: no border state yet)
            if (j) pred = tid ? lexit[tid - 1] : border_in[blockIdx.x - 1];
            need = pred != entry;
        }
        if (!__syncthreads_or(need) || budget == 0) break; // (behind it every lane has read its predecessor; no budget: the file is given up)
        if (rounds == budget) { unfinished = 1; break; }
        if (need) {
            entry = pred;
            const je::Exit x = je::decode_sub(by, st.limit, rec, j, entry, ~0u, none);
            exit = x.state; blocks = x.packed();
            lexit[tid] = exit;
        }
        ++rounds;
    }
    if (active) { a.entry[at] = entry; a.exit[at] = exit; a.count[at] = blocks; }
    const uint32_t last = (st.group + 1 == rec.groups ? rec.subs - st.group * je::kGroupSubs : je::kGroupSubs) - 1;
    if (tid == last) {
        const bool again = budget != 0 && (unfinished || (cold ? st.group + 1 < rec.groups : exit != border_in[blockIdx.x]));
        border_out[blockIdx.x] = exit;
        if (again) atomicAdd(&a.counters[2 * launch], 1u);
        atomicMax(&a.counters[2 * launch + 1], rounds);
        atomicMax(&a.status[st.file].used[(launch & 1) ^ 1], used + rounds); // (every workgroup of the file: the count moves on also where none ran a round)
    }
}

// Inclusive sum over the workgroup's 256 values (lds: 256 words; a barrier is due before they are reused)
__device__ uint32_t group_sum(uint32_t v, uint32_t *lds)
{
    const uint32_t tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < je::kGroupSubs; d <<= 1) {
        const uint32_t t = tid >= d ? lds[tid - d] : 0u;
        __syncthreads();
        lds[tid] += t;
        __syncthreads();
    }
    return lds[tid];
}

__global__ __launch_bounds__(256) void jpeg_entropy_verify_kernel(pixo_dev::JpegEntropyArgs a)
{
    __shared__ uint32_t sums[je::kGroupSubs];
    __shared__ uint32_t best;
    const je::FileRecord &f = a.records[blockIdx.x];
    const uint32_t tid = threadIdx.x, subs = f.subs, first = f.first_sub, want = f.blocks;
    if (tid == 0) best = ~0u;
    uint32_t base = 0; // blocks in front of this chunk
    for (uint32_t j0 = 0; j0 < subs; j0 += je::kGroupSubs) {
        const uint32_t j = j0 + tid;
        const bool active = j < subs;
        uint32_t c = 0, flawed = 0;
        je::State e = je::kDead, x = je::kDead, pred = je::make_state(0, 0, 0);
        if (active) {
            e = a.entry[first + j]; x = a.exit[first + j]; c = a.count[first + j];
            flawed = c >> 31; c &= 0x7FFFFFFFu;
            if (j) pred = a.exit[first + j - 1];
        }
        const uint32_t incl = base + group_sum(c, sums);
        if (active) {
            a.first_block[first + j] = incl - c;
            // what ends the walk at j, in the order a walk lane by lane would see it: 0 not started from its predecessor's exit,
            // 1 the last block completes here, 2 the chain dies here (a dead exit, a flawed lane)
            const uint32_t what = e != pred ? 0u : incl >= want ? 1u : x == je::kDead || flawed ? 2u : 3u;
            if (what < 3) atomicMin(&best, j * 4 + what);
        }
        __syncthreads();
        if (best != ~0u) break;
        base += sums[je::kGroupSubs - 1];
        __syncthreads();
    }
    if (tid == 0) {
        je::FileStatus &s = a.status[blockIdx.x]; // (rounds: the sync launches')
        const uint32_t what = best == ~0u ? 3u : best & 3;
        s.vouched = what == 1;
        s.why = what == 0 ? je::NOT_SETTLED : what == 1 ? je::VOUCHED : what == 2 ? je::CHAIN_DEAD : je::SHORT;
        s.subs = subs;
        s.rounds = s.used[0] > s.used[1] ? s.used[0] : s.used[1];
        s.last_sub = what == 1 ? best >> 2 : 0;
    }
}

__global__ __launch_bounds__(256) void jpeg_entropy_write_kernel(pixo_dev::JpegEntropyArgs a)
{
    __shared__ __attribute__((aligned(16))) je::FileRecord rec;
    __shared__ __attribute__((aligned(16))) uint32_t bytes[je::kStageLds / 4];
    __shared__ uint8_t zigzag[64];
    if (threadIdx.x < 64) zigzag[threadIdx.x] = kZigzagDev[threadIdx.x];
    const Staged st = stage(a.records, a.files, a.scans, &rec, bytes);
    const je::FileStatus &s = a.status[st.file];
    const uint32_t j = st.group * je::kGroupSubs + threadIdx.x;
    if (!s.vouched || j >= rec.subs || j > s.last_sub) return;
    const LdsBytes by{reinterpret_cast<const uint8_t *>(bytes), st.lo};
    const uint32_t first_block = a.first_block[rec.first_sub + j];
    if (first_block >= rec.blocks) return;
    je::WriteSink sink(rec, a.coef, zigzag, first_block);
    (void)je::decode_sub(by, st.limit, rec, j, a.entry[rec.first_sub + j], rec.blocks - first_block, sink);
}

__global__ __launch_bounds__(256) void jpeg_entropy_dc_kernel(pixo_dev::JpegEntropyArgs a)
{
    __shared__ uint32_t sums[je::kGroupSubs];
    const uint32_t file = blockIdx.x / 3, c = blockIdx.x % 3;
    const je::FileRecord &f = a.records[file];
    if (!a.status[file].vouched || c >= f.ncomp) return;
    int16_t *plane = a.coef + f.coef_at[c] / 2;
    const uint32_t n_blocks = f.comp_blocks[c];
    uint32_t carry = 0;
    for (uint32_t n0 = 0; n0 < n_blocks; n0 += je::kGroupSubs) {
        const uint32_t n = n0 + threadIdx.x;
        int16_t *at = nullptr;
        uint32_t v = 0;
        if (n < n_blocks) {
            at = plane + je::coef_index(je::scan_order_block(f, c, n), 0);
            v = static_cast<uint16_t>(*at);
        }
        const uint32_t incl = carry + group_sum(v, sums);
        if (at) *at = static_cast<int16_t>(incl);
        carry += sums[je::kGroupSubs - 1];
        __syncthreads();
    }
}

} // namespace

namespace pixo_dev {

hipError_t launch_jpeg_entropy_sync(const JpegEntropyArgs &a, uint32_t launch, uint32_t cap, hipStream_t stream)
{
    if (a.files == 0 || a.groups == 0 || a.groups > 0x7FFFFFFFu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jpeg_entropy_sync_kernel, dim3(a.groups), dim3(je::kGroupSubs), 0, stream, a, launch, cap);
    return hipGetLastError();
}

hipError_t launch_jpeg_entropy_finish(const JpegEntropyArgs &a, hipStream_t stream)
{
    if (a.files == 0 || a.groups == 0 || a.groups > 0x7FFFFFFFu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jpeg_entropy_verify_kernel, dim3(a.files), dim3(je::kGroupSubs), 0, stream, a);
    hipLaunchKernelGGL(jpeg_entropy_write_kernel, dim3(a.groups), dim3(je::kGroupSubs), 0, stream, a);
    hipLaunchKernelGGL(jpeg_entropy_dc_kernel, dim3(a.files * 3), dim3(je::kGroupSubs), 0, stream, a);
    return hipGetLastError();
}

} // namespace pixo_dev
