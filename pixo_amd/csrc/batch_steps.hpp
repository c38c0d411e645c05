// batch_steps.hpp — the steps the batch drivers (the *_api.cpp files) share, each said once, in the order a driver takes them
// (DESIGN.md §4.0 "Anatomy of a batch driver"): per-record checks, layout, the sub-batch cut, the caller's stream, the job fence,
// the host entries' tail.  Plain functions; every driver still reads top to bottom in its own file.  Host code only: no kernel
// file includes this header.
#pragma once
#include "capi_internal.hpp"

#include <algorithm>

namespace pixo_capi {

// ---- per-record checks -------------------------------------------------------------------------------------------------------
inline std::string where(uint32_t i) { return " (image " + std::to_string(i) + ")"; } // what a batch entry's refusal ends with
int bad_color_type(uint8_t ct, const std::string &where = std::string());               // (context.cpp)
inline uint64_t image_bytes(const pixo_png_image &im) { return static_cast<uint64_t>(im.width) * im.height * bytes_per_pixel(im.color_type); }
// An image of `bytes` bytes at `offset` of a block (an image is at most 2^50 bytes): refused when it starts or ends above 2^62,
// as "batch input too large" or "batch output too large" (`what`); otherwise *furthest moves to its end if that is further.
int record_extent(uint64_t offset, uint64_t bytes, const char *what, const std::string &where, uint64_t *furthest); // (context.cpp)
// The batch entries' first two checks where the batch is one of files
inline int batch_head(const pixo_png_file *files, uint32_t batch)
{
    PIXO_REQUIRE(files);
    return batch_in_range(batch);
}

// ---- layout: the images of a block one behind the other, each at a multiple of 16 ------------------------------------------------
inline uint64_t round16(uint64_t n) { return (n + 15) & ~uint64_t{15}; }
// The next image's record (`reserved` zero) at `at`, which moves on to where the image behind it starts; *end: where this one ends
inline pixo_png_image lay_out(uint64_t &at, uint32_t width, uint32_t height, uint8_t color_type, uint64_t *end)
{
    pixo_png_image im{};
    im.offset = at; im.width = width; im.height = height; im.color_type = color_type;
    *end = at + image_bytes(im);
    at = round16(*end);
    return im;
}
inline void report(const std::vector<pixo_png_image> &laid, pixo_png_image *images) { std::copy(laid.begin(), laid.end(), images); }

// ---- the sub-batch cut: greedy in index order -------------------------------------------------------------------------------
// The budgets are the driver's.  Per image it says whether this one would not fit what the current sub-batch holds; the answer is
// whether a new sub-batch starts at it, and then the driver resets its own counters.  Every sub-batch holds at least one image: the
// first image of one never starts another, whatever its size.
struct SubBatches {
    std::vector<uint32_t> sub_first{0u}; // sub-batch k is images [sub_first[k], sub_first[k + 1]), once closed
    bool starts_at(uint32_t i, bool would_not_fit)
    {
        if (i == sub_first.back() || !would_not_fit) return false;
        sub_first.push_back(i);
        return true;
    }
    void close(uint32_t batch) { sub_first.push_back(batch); }
    uint32_t operator[](size_t k) const { return sub_first[k]; }
    uint32_t back() const { return sub_first.back(); }
    size_t size() const { return sub_first.size(); }                                 // (closed: the sub-batches and the batch's end)
    uint32_t count() const { return static_cast<uint32_t>(sub_first.size() - 1); }   // (closed)
    void report(uint32_t *first, uint32_t *count_out) const                          // what the pixo_hip_debug_*_plan entries hand out
    {
        std::copy(sub_first.begin(), sub_first.end(), first);
        *count_out = count();
    }
};

// ---- the caller's stream (context.cpp) ------------------------------------------------------------------------------------------
// The preamble of a device-pointer entry that enqueues on a stream the caller names: the thread's context bound to the device
// current for the caller (which records the producer stream's event), and that stream ordered behind the producer's work.
int caller_stream_context(void *stream, Context **c, hipStream_t *s);
#define PIXO_CALLER_STREAM_CONTEXT(c, s, stream)                                                        \
    ::pixo_capi::Context *c = nullptr;                                                                  \
    hipStream_t s = nullptr;                                                                            \
    if (const int stream_rc_ = ::pixo_capi::caller_stream_context(stream, &c, &s)) return stream_rc_

// ---- the job fence (context.cpp) ----------------------------------------------------------------------------------------------
// `fence` is the context's event for one family of jobs (each family keeps its own, with its own buffers), recorded behind whatever
// a job has enqueued so far.  Created on first use, then waited for on the host.
int await_last_job(hipEvent_t &fence);

// ---- timed entries: wall time, and events around the device legs of every sub-batch ----------------------------------------------
inline double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
struct BatchLegs {
    std::vector<hipEvent_t> e;
    ~BatchLegs() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    int mark(hipStream_t s)
    {
        hipEvent_t x = nullptr;
        HIP_TRY(hipEventCreate(&x));
        e.push_back(x);
        HIP_TRY(hipEventRecord(x, s));
        return PIXO_OK;
    }
};

// ---- the host entries' tail (host_memory.cpp) -----------------------------------------------------------------------------------
// `n` bytes at d_from come down on the context's stream into a block the caller will own (pixo_hip_free), the stream is waited
// for, *out / *out_len are set; after a failure the block is freed and nothing is set.  Two flavours, and why:
//   download_block   resize and convert.  Their uploads read the CALLER's pixels, so the stream is waited for also when the enqueue
//                    failed (`rc`, handed through).  The block is taken by the entry BEFORE it enqueues the kernels, from
//                    alloc_file alone.  A HIP failure is reported under its call's name.
//   download_pooled  the decoders.  Their uploads read the context's pinned staging, so a failed enqueue returns at once and this
//                    runs only BEHIND a good one.  The block comes from the pinned pool first (the copy down runs at the link's
//                    rate), alloc_file second.  A HIP failure is reported as `what` ("png decode", "png decode batch", "jpeg
//                    decode").  n = 0 (JPEG files of no pixels): a block of one byte, nothing copied.  around: two events, recorded
//                    in front of and behind the copy (the timed entries), or null.
int download_block(Context &c, int rc, uint8_t *block, const void *d_from, size_t n, uint8_t **out, size_t *out_len);
int download_pooled(Context &c, const void *d_from, size_t n, const char *what, uint8_t **out, size_t *out_len, hipEvent_t *around = nullptr);

} // namespace pixo_capi
