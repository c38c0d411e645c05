// host_memory.cpp — the library's host-memory policy for finished files: blocks the caller will own (large ones kept for the
// next large file, a batch's from a pool of pinned memory), huge-page hints, copies into fresh memory over several threads.
#include <malloc.h>
#include <sys/mman.h>

#include <algorithm>

#include "batch_steps.hpp"

namespace pixo_capi {

// Copies into FRESH host memory are page-fault bound (one core maps and fills a few GB/s of new pages):
// above a few MB the bytes are spread over a handful of threads (PIXO_HIP_COPY_THREADS, default 8; 1 = none).
inline unsigned copy_threads() { return debug().copy_threads; }
// A block the caller will own and give back with pixo_hip_free.  Small files: malloc — glibc serves blocks up to its
// (dynamic, <= 32 MB) mmap threshold from recycled heap pages.  Larger ones would be fresh mappings every time, and a
// fresh mapping costs a page fault per 4 KiB when it is first written: for the 178 MB file of a 16384x16384 image that is
// several times the file's whole way over PCIe, and more threads do not help much (the faults serialise on the address
// space; tools/ubench/fresh_pages.cpp).  So pixo_hip_free keeps up to two large blocks instead of unmapping them and the
// next large file reuses one: its pages are resident.  pixo_hip_trim releases them.
constexpr size_t kLargeBlock = size_t{24} << 20;
struct BlockCache {
    std::mutex m;
    struct Entry { void *p; size_t cap; };
    std::vector<Entry> kept;
    static constexpr size_t kMaxKept = 2, kMaxBytes = size_t{1} << 30;
};
BlockCache &block_cache()
{
    static BlockCache *b = new BlockCache;
    return *b;
}
uint8_t *alloc_file(size_t n)
{
    if (n < kLargeBlock || debug().plain_host) return static_cast<uint8_t *>(std::malloc(n ? n : 1));
    {
        BlockCache &bc = block_cache();
        std::lock_guard<std::mutex> lock(bc.m);
        size_t best = bc.kept.size();
        for (size_t i = 0; i < bc.kept.size(); ++i) // smallest block that holds the file and is not absurdly larger
            if (bc.kept[i].cap >= n && bc.kept[i].cap <= 2 * n + kLargeBlock && (best == bc.kept.size() || bc.kept[i].cap < bc.kept[best].cap)) best = i;
        if (best < bc.kept.size()) {
            void *p = bc.kept[best].p;
            bc.kept.erase(bc.kept.begin() + static_cast<long>(best));
            return static_cast<uint8_t *>(p);
        }
    }
    // a fresh block: 2 MiB aligned with a transparent-huge-page hint — filled by big_copy's threads it costs 2.7 ms for 178 MB
    // on the GPU box where plain malloc'd pages cost 15 (one thread: 28); a recycled block 1.7 (tools/ubench/fresh_pages.cpp,
    // profiles/r03_fresh_pages.txt).  Head-room: the next file of about this size fits the recycled block.
    constexpr size_t kHuge = size_t{2} << 20;
    const size_t rounded = (n + n / 8 + kHuge - 1) / kHuge * kHuge;
    void *p = nullptr;
    if (posix_memalign(&p, kHuge, rounded) != 0) return nullptr;
    (void)madvise(p, rounded, MADV_HUGEPAGE);
    return static_cast<uint8_t *>(p);
}
// ---- files of a BATCH that the caller will own (pixo_hip_jpeg_encode_batch_device) -------------------------------
// 64 x 1.4 MB of fresh malloc'd pages are 22,000 page faults: 26 ms for a batch whose kernels take 0.45 and whose bytes cross PCIe
// in 1.7.  glibc does not keep such blocks either (they are mmap'ed or trimmed off the heap's top).  So the blocks of a batch's
// files come from a pool of PINNED host memory that pixo_hip_free gives back to: resident pages, and the device-to-host copy of a
// file lands in the caller's block directly — no staging buffer, no second pass.  To the caller a block is ordinary host memory
// it owns until pixo_hip_free.  At most kMaxTotal bytes; beyond that (or with debug switch plain_host) plain malloc as before.
struct PinnedPool {
    std::mutex m;
    struct Block { void *p; size_t cap; bool used; };
    std::vector<Block> blocks;
    size_t total = 0;
    static constexpr size_t kMaxTotal = size_t{2} << 30, kGrain = size_t{256} << 10;
};
PinnedPool &pinned_pool()
{
    static PinnedPool *pp = new PinnedPool; // (never destroyed: no HIP call in a static destructor)
    return *pp;
}
uint8_t *pool_take(size_t n)
{
    if (debug().plain_host) return nullptr;
    PinnedPool &pp = pinned_pool();
    std::lock_guard<std::mutex> lock(pp.m);
    size_t best = pp.blocks.size();
    for (size_t i = 0; i < pp.blocks.size(); ++i) // the smallest free block that holds the file and is not absurdly larger
        if (!pp.blocks[i].used && pp.blocks[i].cap >= n && pp.blocks[i].cap <= 2 * n + (size_t{1} << 20) &&
            (best == pp.blocks.size() || pp.blocks[i].cap < pp.blocks[best].cap)) best = i;
    if (best < pp.blocks.size()) {
        pp.blocks[best].used = true;
        return static_cast<uint8_t *>(pp.blocks[best].p);
    }
    const size_t cap = (n + n / 8 + PinnedPool::kGrain) / PinnedPool::kGrain * PinnedPool::kGrain; // (head-room: the next batch's file fits)
    if (pp.total + cap > PinnedPool::kMaxTotal) return nullptr;
    void *p = nullptr;
    if (hipHostMalloc(&p, cap, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    pp.blocks.push_back({p, cap, true});
    pp.total += cap;
    return static_cast<uint8_t *>(p);
}
bool pool_give(void *p)
{
    PinnedPool &pp = pinned_pool();
    std::lock_guard<std::mutex> lock(pp.m);
    for (PinnedPool::Block &b : pp.blocks)
        if (b.p == p) { b.used = false; return true; }
    return false;
}
void pool_drain()
{ // (pixo_hip_trim) the blocks nobody holds go back to the driver
    PinnedPool &pp = pinned_pool();
    std::lock_guard<std::mutex> lock(pp.m);
    std::vector<PinnedPool::Block> keep;
    for (const PinnedPool::Block &b : pp.blocks) {
        if (b.used) keep.push_back(b);
        else { (void)hipHostFree(b.p); pp.total -= b.cap; }
    }
    pp.blocks.swap(keep);
}

void free_file(void *p)
{
    if (!p) return;
    if (pool_give(p)) return;
    const size_t cap = debug().plain_host ? 0 : malloc_usable_size(p);
    if (cap >= kLargeBlock) {
        BlockCache &bc = block_cache();
        std::lock_guard<std::mutex> lock(bc.m);
        size_t bytes = cap;
        for (const BlockCache::Entry &e : bc.kept) bytes += e.cap;
        if (bc.kept.size() < BlockCache::kMaxKept && bytes <= BlockCache::kMaxBytes) {
            bc.kept.push_back({p, cap});
            return;
        }
    }
    std::free(p);
}
void drop_kept_blocks()
{
    pool_drain();
    BlockCache &bc = block_cache();
    std::lock_guard<std::mutex> lock(bc.m);
    for (const BlockCache::Entry &e : bc.kept) std::free(e.p);
    bc.kept.clear();
}

// Transparent huge pages for the whole 2 MiB units inside [p, p + n): a hint before the first touch of a large block the
// CALLER allocated (a fresh 178 MB block is 43,000 page faults otherwise: 15 ms over 8 threads against 2.7 with huge pages,
// profiles/r03_fresh_pages.txt; resident pages are not affected).
void advise_huge(void *p, size_t n)
{
    constexpr uintptr_t kHuge = uintptr_t{2} << 20;
    const uintptr_t a = (reinterpret_cast<uintptr_t>(p) + kHuge - 1) & ~(kHuge - 1), b = (reinterpret_cast<uintptr_t>(p) + n) & ~(kHuge - 1);
    if (n >= kLargeBlock && b > a && !debug().plain_host) (void)madvise(reinterpret_cast<void *>(a), b - a, MADV_HUGEPAGE);
}

void big_copy(uint8_t *dst, const uint8_t *src, size_t n)
{
    advise_huge(dst, n);
    constexpr size_t kSlice = size_t{1} << 20;
    const size_t slices = (n + kSlice - 1) / kSlice;
    const unsigned t = static_cast<unsigned>(std::min<size_t>(copy_threads(), slices / 2));
    if (t <= 1) { std::memcpy(dst, src, n); return; }
    run_on_threads(t, [&](unsigned i) {
        const size_t a = slices * i / t * kSlice, b = std::min(n, slices * (i + 1) / t * kSlice);
        if (b > a) std::memcpy(dst + a, src + a, b - a);
    });
}

// ... and into memory the caller owns: a fresh malloc block, or storage it supplied
int deliver(const uint8_t *file, size_t n, uint8_t **out, size_t *out_len)
{
    uint8_t *p = alloc_file(n);
    if (!p) return fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
    big_copy(p, file, n);
    *out = p;
    *out_len = n;
    return PIXO_OK;
}

int hand_over(const std::vector<uint8_t> &v, uint8_t **out, size_t *out_len)
{
    uint8_t *p = alloc_file(v.size());
    if (!p) return fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
    big_copy(p, v.data(), v.size());
    *out = p;
    *out_len = v.size();
    return PIXO_OK;
}

// ---- the host entries' tail (batch_steps.hpp says which entries take which, and why) ------------------------------------------
int download_block(Context &c, int rc, uint8_t *block, const void *d_from, size_t n, uint8_t **out, size_t *out_len)
{
    if (!rc) {
        const hipError_t e = hipMemcpyAsync(block, d_from, n, hipMemcpyDeviceToHost, c.stream);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
    }
    const hipError_t e = hipStreamSynchronize(c.stream); // (also after a failure: the uploads read the caller's pixels)
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    if (rc) { free_file(block); return rc; }
    *out = block;
    *out_len = n;
    return PIXO_OK;
}

int download_pooled(Context &c, const void *d_from, size_t n, const char *what, uint8_t **out, size_t *out_len, hipEvent_t *around)
{
    uint8_t *block = pool_take(std::max<size_t>(n, 1));
    if (!block) block = alloc_file(std::max<size_t>(n, 1));
    if (!block) return fail(PIXO_ERR_COMPRESSION, "Compression error: out of host memory");
    hipError_t e = around ? hipEventRecord(around[0], c.stream) : hipSuccess;
    if (e == hipSuccess && n) e = hipMemcpyAsync(block, d_from, n, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess && around) e = hipEventRecord(around[1], c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) { free_file(block); return hip_fail(e, what); }
    *out = block;
    *out_len = n;
    return PIXO_OK;
}

} // namespace pixo_capi
