// png_api.cpp — the extern "C" PNG row-filter entry points (config 5: apply_filters + the zlib wrapper's Adler-32).
#include "capi_internal.hpp"
#include "png_filter.hpp"

#include <algorithm>
#include <vector>

using namespace pixo_capi;

namespace pixo_capi {
int png_plan(uint32_t width, uint32_t height, uint64_t area, uint32_t bpp, uint8_t strategy, uint32_t flags, int *run, bool *sequential_fast)
{
    if (width == 0 || height == 0) return bad_dimensions(width, height);
    if (!(bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8))
        return fail(PIXO_ERR_UNSUPPORTED_COLOR_TYPE, "Unsupported color type for this format");
    if (strategy > PIXO_PNG_BIGRAMS) return fail(PIXO_ERR_COMPRESSION, "Compression error: unknown PNG filter strategy");
    int s = strategy;
    const bool adaptive = s == PIXO_PNG_ADAPTIVE || s == PIXO_PNG_ADAPTIVE_FAST || s == PIXO_PNG_BIGRAMS;
    if (area <= 4096 && adaptive) s = PIXO_PNG_SUB; // src/png/filter.rs:76-86
    // the stateful AdaptiveFast runs wherever the reference does not take its rayon path (:94-112)
    *sequential_fast = s == PIXO_PNG_ADAPTIVE_FAST && ((flags & PIXO_PNG_NO_RAYON) || height <= 32);
    *run = s;
    return PIXO_OK;
}
} // namespace pixo_capi

namespace {
// zlib Adler-32 of the filtered stream from the per-row sums (A = byte sum, B = sum of
// (row_len - i) * byte_i): s2 += row_len * s1 + B, s1 += A  (mod 65521)
uint32_t combine_adler(const unsigned long long *sums, uint32_t height, uint64_t out_row_bytes)
{
    const uint64_t M = 65521;
    uint64_t s1 = 1, s2 = 0;
    const uint64_t L = out_row_bytes % M;
    for (uint32_t y = 0; y < height; ++y) {
        s2 = (s2 + L * s1 + sums[2 * y + 1] % M) % M;
        s1 = (s1 + sums[2 * y] % M) % M;
    }
    return static_cast<uint32_t>((s2 << 16) | s1);
}

// The per-row sums on the device, their copy on the host, the kernels' scratch word
int reserve_sums(Context &c, uint32_t height)
{
    int rc;
    if ((rc = c.p_sums.reserve(static_cast<size_t>(height) * 16)) || (rc = c.h_sums.reserve(static_cast<size_t>(height) * 16))) return rc;
    return c.p_scratch.reserve(16);
}

} // namespace

int pixo_capi::png_filter_on_device(Context &c, const void *d_in, uint32_t width, uint32_t height, uint32_t bpp, int run,
                                    bool sequential_fast, void *d_out, uint32_t *adler)
{
    if (const int rc = reserve_sums(c, height)) return rc;
    HIP_TRY(pixo_dev::launch_png_filter(d_in, width, height, bpp, run, sequential_fast, d_out,
                                        c.p_sums.as<unsigned long long>(), c.p_scratch.as<int>(), c.stream));
    HIP_TRY(hipMemcpyAsync(c.h_sums.p, c.p_sums.p, static_cast<size_t>(height) * 16, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    *adler = combine_adler(c.h_sums.as<unsigned long long>(), height, static_cast<uint64_t>(width) * bpp + 1);
    return PIXO_OK;
}

// The batch form (png_encode_api.cpp): one launch over the rows of `batch` images, all row sums on their way down in one
// copy.  Nothing is waited for here; png_filter_batch_adler reads the sums once the stream has been synchronised.
int pixo_capi::png_filter_batch_begin(Context &c, const void *d_in, uint32_t width, uint32_t height, uint32_t batch, uint32_t bpp, int run, void *d_out)
{
    const uint64_t rows = static_cast<uint64_t>(height) * batch;
    if (rows > 0x7FFFFFFFull) return hip_fail(hipErrorInvalidValue, "rows of a PNG batch");
    if (const int rc = reserve_sums(c, static_cast<uint32_t>(rows))) return rc;
    HIP_TRY(pixo_dev::launch_png_filter_batch(d_in, width, height, batch, bpp, run, d_out, c.p_sums.as<unsigned long long>(), c.stream));
    HIP_TRY(hipMemcpyAsync(c.h_sums.p, c.p_sums.p, static_cast<size_t>(rows) * 16, hipMemcpyDeviceToHost, c.stream));
    return PIXO_OK;
}
uint32_t pixo_capi::png_filter_batch_adler(const Context &c, uint64_t sums_at, uint32_t height, uint64_t row_bytes)
{
    return combine_adler(c.h_sums.as<unsigned long long>() + 2 * static_cast<size_t>(sums_at), height, row_bytes + 1);
}

// The ragged form (png_encode_api.cpp png_images): the records of all classes in one upload, one launch per class, the sums
// of all rows in one copy down.  The pinned table is written only after the stream has drained what read it last: every
// caller has waited for its previous sub-batch's files by then.
int pixo_capi::png_filter_images_begin(Context &c, const void *d_in, const std::vector<pixo_png_images::Item> &items, void *d_out, uint32_t *launches)
{
    namespace im = pixo_png_images;
    std::vector<im::Record> table;
    std::vector<im::Launch> plan;
    std::vector<uint32_t> record_item;
    uint64_t rows = 0;
    for (const im::Item &it : items) rows += it.height;
    if (items.empty() || rows > 0x7FFFFFFFull || !im::build_table(items, reinterpret_cast<uintptr_t>(d_in), table, plan, record_item))
        return hip_fail(hipErrorInvalidValue, "rows of a PNG batch");
    const size_t bytes = table.size() * sizeof(im::Record);
    int rc;
    if ((rc = reserve_sums(c, static_cast<uint32_t>(rows))) || (rc = c.p_images.reserve(bytes)) || (rc = c.h_images.reserve(bytes))) return rc;
    std::memcpy(c.h_images.p, table.data(), bytes);
    HIP_TRY(hipMemcpyAsync(c.p_images.p, c.h_images.p, bytes, hipMemcpyHostToDevice, c.stream));
    for (const im::Launch &l : plan)
        HIP_TRY(pixo_dev::launch_png_filter_images(d_in, d_out, c.p_sums.as<unsigned long long>(), c.p_images.as<im::Record>() + l.first_record, l, c.stream));
    HIP_TRY(hipMemcpyAsync(c.h_sums.p, c.p_sums.p, static_cast<size_t>(rows) * 16, hipMemcpyDeviceToHost, c.stream));
    *launches = static_cast<uint32_t>(plan.size());
    return PIXO_OK;
}

namespace {
// A large image from host pixels to caller storage, band by band (round 3).  Rows are independent once the row above is on
// the device, so: the calling thread uploads bands of ~8 MiB back to back on the upload stream (a pageable source blocks it
// for the copy's duration anyway); each band's kernel and the download of its filtered rows into the context's PINNED
// buffer follow on the context's stream as soon as the band has arrived; and while the next band uploads, the band before
// last is copied on into the caller's storage by the library's copy threads (huge-page hint first: the result array of
// a call is usually fresh).  A device-to-host copy straight into that pageable storage made the runtime fault in and pin
// its pages as it went: 30-39 ms for the 67 MB of a 4096x4096 RGBA image whose bytes need 1.3 ms each way on the link.
// The stateful AdaptiveFast (row 0 decides for all) runs as one launch after the whole upload.
int png_filter_in_bands(Context &c, const uint8_t *data, uint32_t width, uint32_t height, uint32_t bpp, int run, bool seq,
                        uint8_t *out, uint32_t *adler)
{
    const size_t row_in = static_cast<size_t>(width) * bpp, row_out = row_in + 1;
    const size_t out_bytes = row_out * height;
    int rc = c.h_file.reserve(out_bytes);
    if (rc) { // (the pinned staging is an optimisation — a 16384x16384 RGBA image wants 1.3 GB of it.  Without it:
              // the whole image in one go, its rows straight into the caller's storage, as before round 3)
        (void)hipGetLastError();
        HIP_TRY(hipMemcpyAsync(c.p_in.p, data, row_in * height, hipMemcpyHostToDevice, c.stream));
        if ((rc = png_filter_on_device(c, c.p_in.p, width, height, bpp, run, seq, c.p_out.p, adler))) return rc;
        HIP_TRY(hipMemcpy(out, c.p_out.p, out_bytes, hipMemcpyDeviceToHost));
        return PIXO_OK;
    }
    if ((rc = reserve_sums(c, height))) return rc;
    if (!c.upload_stream) HIP_TRY(hipStreamCreateWithFlags(&c.upload_stream, hipStreamNonBlocking));
    advise_huge(out, out_bytes);
    const uint32_t band_rows = seq ? height : static_cast<uint32_t>(std::max<size_t>(1, (size_t{8} << 20) / row_in));
    const uint32_t bands = (height + band_rows - 1) / band_rows;
    std::vector<hipEvent_t> up(bands, nullptr), down(bands, nullptr);
    hipError_t e = hipSuccess;
    auto copy_on = [&](uint32_t b) { // band b's filtered rows: pinned buffer -> the caller's storage
        e = hipEventSynchronize(down[b]);
        const size_t off = static_cast<size_t>(b) * band_rows * row_out;
        const size_t n = std::min(static_cast<size_t>(band_rows) * row_out, out_bytes - off);
        if (e == hipSuccess) big_copy(out + off, c.h_file.as<uint8_t>() + off, n);
    };
    for (uint32_t b = 0; b < bands && e == hipSuccess; ++b) {
        const uint32_t r0 = b * band_rows, rows = std::min(band_rows, height - r0);
        e = hipEventCreateWithFlags(&up[b], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&down[b], hipEventDisableTiming);
        if (e == hipSuccess) e = hipMemcpyAsync(static_cast<uint8_t *>(c.p_in.p) + r0 * row_in, data + r0 * row_in, rows * row_in, hipMemcpyHostToDevice, c.upload_stream);
        if (e == hipSuccess) e = hipEventRecord(up[b], c.upload_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(c.stream, up[b], 0);
        if (e == hipSuccess) e = pixo_dev::launch_png_filter_rows(c.p_in.p, width, height, bpp, run, seq, c.p_out.p, c.p_sums.as<unsigned long long>(),
                                                                  c.p_scratch.as<int>(), r0, rows, c.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c.h_file.as<uint8_t>() + r0 * row_out, static_cast<const uint8_t *>(c.p_out.p) + r0 * row_out, rows * row_out, hipMemcpyDeviceToHost, c.stream);
        if (e == hipSuccess) e = hipEventRecord(down[b], c.stream);
        if (e == hipSuccess && b >= 2) copy_on(b - 2);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(c.h_sums.p, c.p_sums.p, static_cast<size_t>(height) * 16, hipMemcpyDeviceToHost, c.stream);
    for (uint32_t b = bands >= 2 ? bands - 2 : 0; b < bands && e == hipSuccess; ++b) copy_on(b);
    const hipError_t e2 = hipStreamSynchronize(c.stream); // (also after an error: nothing of ours in flight when the events go)
    (void)hipStreamSynchronize(c.upload_stream);
    if (e == hipSuccess) e = e2;
    for (hipEvent_t ev : up) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : down) if (ev) (void)hipEventDestroy(ev);
    if (e != hipSuccess) return hip_fail(e, "PNG filter stage in bands");
    *adler = combine_adler(c.h_sums.as<unsigned long long>(), height, row_out);
    return PIXO_OK;
}
} // namespace

extern "C" {

int pixo_hip_png_filter(const uint8_t *data, size_t data_len, uint32_t width, uint32_t height, uint32_t bytes_per_pixel,
                        uint8_t strategy, uint32_t flags, uint8_t *out, size_t out_capacity, uint32_t *adler32)
{
    CallerStorageScope storage(out && out_capacity);
    int run = 0;
    bool seq = false;
    int rc = png_plan(width, height, static_cast<uint64_t>(width) * height, bytes_per_pixel, strategy, flags, &run, &seq);
    if (rc) return rc;
    const size_t in_bytes = static_cast<size_t>(width) * height * bytes_per_pixel;
    const size_t out_bytes = static_cast<size_t>(height) * (static_cast<size_t>(width) * bytes_per_pixel + 1);
    if (data_len != in_bytes) return bad_length(in_bytes, data_len);
    if (out_capacity < out_bytes) return too_small(out_bytes);
    if (!data || !out || !adler32) return fail(PIXO_ERR_COMPRESSION, "Compression error: null argument");
    PIXO_THREAD_CONTEXT(c);
    if (out_bytes < (size_t{4} << 20)) { // small: one copy each way
        if ((rc = upload(c, c.p_in, data, in_bytes)) || (rc = c.p_out.reserve(out_bytes))) return rc;
        if ((rc = png_filter_on_device(c, c.p_in.p, width, height, bytes_per_pixel, run, seq, c.p_out.p, adler32))) return rc;
        HIP_TRY(hipMemcpy(out, c.p_out.p, out_bytes, hipMemcpyDeviceToHost));
        return PIXO_OK;
    }
    if ((rc = reserve16(c.p_in, in_bytes)) || (rc = c.p_out.reserve(out_bytes))) return rc;
    return png_filter_in_bands(c, data, width, height, bytes_per_pixel, run, seq, out, adler32);
}

int pixo_hip_png_filter_async(const void *d_data, uint32_t width, uint32_t height, uint32_t bytes_per_pixel,
                              uint8_t strategy, uint32_t flags, void *d_out, void *d_row_sums, void *d_scratch,
                              void *stream)
{
    int run = 0;
    bool seq = false;
    int rc = png_plan(width, height, static_cast<uint64_t>(width) * height, bytes_per_pixel, strategy, flags, &run, &seq);
    if (rc) return rc;
    HIP_TRY(pixo_dev::launch_png_filter(d_data, width, height, bytes_per_pixel, run, seq, d_out,
                                        static_cast<unsigned long long *>(d_row_sums), static_cast<int *>(d_scratch),
                                        static_cast<hipStream_t>(stream)));
    return PIXO_OK;
}

uint32_t pixo_hip_png_adler32_from_row_sums(const uint64_t *row_sums, uint32_t width, uint32_t height,
                                            uint32_t bytes_per_pixel)
{
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64");
    return combine_adler(reinterpret_cast<const unsigned long long *>(row_sums), height,
                         static_cast<uint64_t>(width) * bytes_per_pixel + 1);
}

int pixo_hip_png_filter_device(const void *d_data, uint32_t width, uint32_t height, uint32_t bytes_per_pixel,
                               uint8_t strategy, uint32_t flags, void *d_out, uint32_t *adler32)
{
    int run = 0;
    bool seq = false;
    int rc = png_plan(width, height, static_cast<uint64_t>(width) * height, bytes_per_pixel, strategy, flags, &run, &seq);
    if (rc) return rc;
    PIXO_REQUIRE(d_data);
    PIXO_REQUIRE(d_out);
    PIXO_REQUIRE(adler32);
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return png_filter_on_device(*c, d_data, width, height, bytes_per_pixel, run, seq, d_out, adler32);
}

} // extern "C"
