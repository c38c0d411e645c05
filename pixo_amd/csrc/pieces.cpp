// pieces.cpp — a scan coded in PIECES so that the file's way to the host overlaps the coding (when: baseline_plan.hpp), and the
// context's copy helper thread that uploads and sends the pieces of host pixels.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>

#include "capi_internal.hpp"

namespace pixo_capi {

// One uninterrupted scan of a large image, coded in PIECES so that the file's way to the host (0.21 of the 0.31 ms of a
// 4096x4096 noise image, 3.3 of 4.4 ms for 16384x16384) overlaps the coding: piece k = a run of consecutive groups,
// coded and stuffed by its own launch pair; the pieces hand each other the bit position and the byte position on the
// device (pixo_dev::ScanPiece), the host only waits for piece k's event to learn how many bytes it may copy — on a second
// stream — while piece k + 1 is being coded.  The bytes are the same as from one launch pair; a piece whose stream
// outgrows the guess its stuffing grid was sized for, or an output buffer that proves too small, sends the caller back
// to the one-piece path (return value 1; nothing of the result is kept).
constexpr uint32_t kMaxPieces = 16;
// Piece sizes (debug switches piece_groups / piece_medium / piece_schedule, capi_internal.hpp; which scans: baseline_plan.hpp):
//  * large scans: equal pieces of at least debug().piece_groups (2048) groups of 192 blocks, at most kMaxPieces of them;
//  * medium scans (debug().piece_medium (1024) <= groups < 2 piece_groups): a few pieces that GROW, relative sizes
//    debug().piece_schedule ("1:3").  4096x4096 noise, 11 MB file, into pinned memory: one piece 0.313 ms, "1:3" 0.301,
//    "1:2:5" 0.302, "1:2:3:4" 0.315; with the coefficient kernel band by band as well: "1:3" 0.291, "1:2:5" 0.299, "1:5" 0.310
//    (tools/gpu/r2w.sh): the first piece's bytes leave 60 us after the start instead of 100, the rest is the file's
//    0.21 ms on PCIe.
inline uint64_t piece_min_groups() { return debug().piece_groups; }
inline const std::vector<uint32_t> &piece_schedule() { return debug().piece_schedule; }

} // namespace pixo_capi

// A context's second host thread.  A copy from or to PAGEABLE host memory keeps the calling thread inside the runtime until
// the bytes have moved (it stages them through pinned buffers): one thread can therefore not keep both directions of the
// PCIe link busy — 48 MiB in + 11 MiB out take 1.11 ms from one thread and 0.93 ms from two (tools/ubench/duplex.cpp,
// profiles/r03_duplex_copies.txt).  The helper runs one job at a time for its context; it lives as long as the process.
struct pixo_capi::CopyHelper {
    std::mutex m;
    std::condition_variable cv, idle;
    std::function<void()> job;
    bool has_job = false, busy = false, stop = false;
    std::thread th;
    CopyHelper() : th([this] { loop(); }) {}
    // (a context that is deleted — excess contexts of the pool, pixo_hip_trim — takes its helper thread with it;
    // it used to stay behind, blocked on its condition variable, one per deleted context)
    ~CopyHelper()
    {
        {
            std::lock_guard<std::mutex> lock(m);
            stop = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
    void loop()
    {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lock(m);
                cv.wait(lock, [&] { return has_job || stop; });
                if (!has_job) return; // (stop)
                f.swap(job);
                has_job = false;
            }
            f();
            {
                std::lock_guard<std::mutex> lock(m);
                busy = false;
            }
            idle.notify_all();
        }
    }
    void start(std::function<void()> f)
    {
        {
            std::lock_guard<std::mutex> lock(m);
            job = std::move(f);
            has_job = busy = true;
        }
        cv.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> lock(m);
        idle.wait(lock, [&] { return !busy; });
    }
};

namespace pixo_capi {

void destroy_copy_helper(CopyHelper *h) { delete h; }

int device_entropy_pieces(Context &c, ScanJob &j, hipStream_t stream, uint8_t *dst, size_t dst_cap, uint64_t *scan_bytes,
                          const PixelSource *src)
{ // dst: where the stuffed scan goes on the host (dst_cap bytes available); tables are uploaded, j.a is set up
    namespace pd = pixo_dev;
    note_route(route::PIECES | route::TWO_KERNEL | route::SINGLE_PASS_TUPLE | (src && src->host_px ? route::HOST_BANDS : 0));
    const uint64_t kGroupBlocks = 192, groups = (j.n + kGroupBlocks - 1) / kGroupBlocks;
    // where the pieces begin (in groups).  A large scan: equal pieces of at least piece_min_groups().  A medium one (a
    // 4096x4096 image): a few pieces that GROW — the first small, so that its bytes leave early, each next one coded
    // while the one before travels (weights from piece_schedule()).
    uint64_t begin[kMaxPieces + 1];
    uint32_t pieces = 0;
    const bool from_host = src && src->host_px;
    if (from_host) { // pixels still in host memory: pieces sized for the UPLOAD pipeline — about 12 MB of pixels each, so that
        // a band's kernels (tens of microseconds) disappear behind the next band's way over PCIe (>= 100 us)
        const uint64_t px_bytes = pixel_bytes(*src->o, *src->g);
        const uint32_t want = static_cast<uint32_t>(std::min<uint64_t>(kMaxPieces, std::max<uint64_t>(2, px_bytes / (uint64_t{debug().bands_upload_mb} << 20))));
        for (uint32_t k = 0; k < want; ++k) {
            const uint64_t g0 = groups * k / want;
            if (pieces == 0 || g0 > begin[pieces - 1]) begin[pieces++] = g0;
        }
    } else if (groups >= 2 * piece_min_groups()) {
        const uint64_t per = std::max<uint64_t>((groups + kMaxPieces - 1) / kMaxPieces, piece_min_groups());
        for (uint64_t g0 = 0; g0 < groups; g0 += per) begin[pieces++] = g0; // (none is empty)
    } else {
        const std::vector<uint32_t> &w = piece_schedule();
        uint64_t sum = 0, acc = 0;
        for (uint32_t x : w) sum += x;
        for (size_t i = 0; i < w.size() && pieces < kMaxPieces; ++i) {
            const uint64_t g0 = groups * acc / sum;
            if (pieces == 0 || g0 > begin[pieces - 1]) begin[pieces++] = g0;
            acc += w[i];
        }
    }
    begin[pieces] = groups;
    // coefficient bands in front of the pieces: only where a piece can begin with an MCU row (the groups of 192 blocks and
    // the MCU rows must share boundaries: 4:2:0 widths that are multiples of 512, 4:4:4 of 512, gray of 1536)
    uint64_t groups_per_row = 0;
    if (src) {
        const uint32_t unit = (!src->g->gray && src->g->s420) ? 16u : 8u, units_x = (src->o->width + unit - 1) / unit;
        const uint64_t row_blocks = static_cast<uint64_t>(units_x) * j.a.blocks_per_mcu;
        if (row_blocks % kGroupBlocks == 0) {
            groups_per_row = row_blocks / kGroupBlocks;
            uint32_t kept = 1; // (piece 0 begins at row 0)
            for (uint32_t k = 1; k < pieces; ++k) {
                const uint64_t g0 = begin[k] / groups_per_row * groups_per_row;
                if (g0 > begin[kept - 1]) begin[kept++] = g0;
            }
            pieces = kept;
            begin[pieces] = groups;
        } else { // (no common boundaries: the whole image first)
            if (from_host) {
                HIP_TRY(hipMemcpyAsync(const_cast<void *>(src->d_px), src->host_px, pixel_bytes(*src->o, *src->g), hipMemcpyHostToDevice, stream));
            }
            const int rc = coeffs_rows(c, src->d_px, *src->o, *src->g, stream, src->dy, src->dcb, src->dcr, 0, 0);
            if (rc) return rc;
        }
    }
    const bool upload_bands = from_host && groups_per_row != 0;
    if (upload_bands) {
        if (!c.upload_stream) HIP_TRY(hipStreamCreateWithFlags(&c.upload_stream, hipStreamNonBlocking));
        while (c.band_up.size() < pieces) {
            hipEvent_t e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            c.band_up.push_back(e);
        }
    }
    if (!c.copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c.copy_stream, hipStreamNonBlocking));
    while (c.piece_done.size() < pieces) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c.piece_done.push_back(e);
    }
    if (const int rc = c.e_chain.reserve(2 * (kMaxPieces + 1) * 8)) return rc;
    unsigned long long *bits_chain = c.e_chain.as<unsigned long long>(), *out_chain = bits_chain + kMaxPieces + 1;
    const size_t out_cap = std::max<size_t>(j.stream_cap / 4, 4096);
    if (const int rc = c.e_out.reserve(out_cap)) return rc;
    // every piece has its own part of the stream buffer (a block has at most 209 bytes; 64 bytes of slack per piece)
    struct Piece { uint64_t first_block, blocks, tiles; uint32_t *stream; };
    Piece pc[kMaxPieces];
    for (uint32_t k = 0; k < pieces; ++k) {
        pc[k].first_block = std::min<uint64_t>(j.n, begin[k] * kGroupBlocks);
        pc[k].blocks = std::min<uint64_t>(j.n, begin[k + 1] * kGroupBlocks) - pc[k].first_block;
        pc[k].tiles = pd::stuff_tiles(pc[k].blocks * 64 + 4096);
    }
    if (const int rc = c.e_stream.reserve(j.stream_cap + 80 * kMaxPieces)) return rc;
    for (uint32_t k = 0; k < pieces; ++k) pc[k].stream = c.e_stream.as<uint32_t>() + (pc[k].first_block * 209 + 64 * k + 15) / 16 * 4;
    const size_t state_words = pd::fused_code_state_words(j.n);
    Stopwatch sw;
    uint64_t done = 0; // bytes of the scan that are on their way to the host
    bool redo = false, gave_up = false;
    uint32_t next_out = 0; // first piece whose bytes have not been sent yet
    // piece k has been coded (its event has fired): its bytes onto the copy stream, unless something went wrong
    Stopwatch sw_send; // (send_piece may run on the helper thread: a stopwatch of its own)
    auto send_piece = [&](uint32_t k) -> int {
        if (redo) return PIXO_OK; // (everything that was enqueued is still waited for)
        const uint64_t *mail = c.mail->totals + 4 * k;
        if (mail[3]) { redo = gave_up = true; return PIXO_OK; } // (a kernel of this piece gave up waiting: the later pieces follow suit)
        const uint64_t stream_bits = mail[0], packed = k + 1 != pieces ? stream_bits / 8 : (stream_bits + 7) / 8;
        if (pd::stuff_tiles(packed) > pc[k].tiles) { redo = true; return PIXO_OK; } // (the stuffing grid was a guess: this piece is not complete)
        const uint64_t bytes = mail[1];
        if (done + bytes > c.e_out.cap || done + bytes > dst_cap) { redo = true; return PIXO_OK; }
        if (bytes) HIP_TRY(hipMemcpyAsync(dst + done, c.e_out.as<uint8_t>() + done, bytes, hipMemcpyDeviceToHost, c.copy_stream));
        done += bytes;
        sw_send.lap("  copy enqueued");
        return PIXO_OK;
    };
    // piece k: its MCU rows through the coefficient kernel (where the pieces follow the rows), then the two entropy kernels
    auto launch_piece = [&](uint32_t k) -> int {
        pd::ScanArgs a = j.a;
        a.nblocks = pc[k].blocks;
        a.pad_last = k + 1 == pieces ? 1u : 0u;
        const pd::ScanPiece piece{pc[k].first_block, k, bits_chain, k ? pc[k - 1].stream : nullptr};
        unsigned long long *mail = mailbox(c) + 4 * k;
        const bool zero = c.e_code_state.known >= state_words;
        c.e_code_state.known = 0;
        if (groups_per_row) {
            const uint32_t row0 = static_cast<uint32_t>(begin[k] / groups_per_row);
            const uint32_t rows = k + 1 == pieces ? 0u : static_cast<uint32_t>(begin[k + 1] / groups_per_row) - row0;
            if (upload_bands) HIP_TRY(hipStreamWaitEvent(stream, c.band_up[k], 0)); // (its pixels arrive on the upload stream)
            const int rc = coeffs_rows(c, src->d_px, *src->o, *src->g, stream, src->dy, src->dcb, src->dcr, row0, rows);
            if (rc) return rc;
        }
        HIP_TRY(pd::launch_scan_code(a, c.e_code_state.as<unsigned long long>(), zero, pc[k].stream, c.e_stuff_state.as<unsigned long long>(),
                                     pd::fused_stuff_state_words(j.stream_cap), mail, stream, &piece, nullptr, debug().spin_budget));
        HIP_TRY(pd::launch_stuff_fused(pc[k].stream, c.e_code_state.as<unsigned long long>(), state_words, 0, /*band=*/k + 1 != pieces,
                                       j.stream_cap, 0, pc[k].tiles, c.e_stuff_state.as<unsigned long long>(), /*state_is_zero=*/true,
                                       c.e_out.as<uint8_t>(), c.e_out.cap, mail, stream, out_chain, k, nullptr, debug().spin_budget));
        c.e_code_state.known = state_words;
        HIP_TRY(hipEventRecord(c.piece_done[k], stream));
        return PIXO_OK;
    };
    if (upload_bands) {
        // Pixels from the host.  A copy from pageable memory keeps the calling thread inside the runtime until the bytes have
        // moved, and whatever else that thread has to do in between — launches, events — is time the link stands still.  So
        // THIS thread does nothing but enqueue the bands' uploads back to back; the context's helper thread follows it band
        // by band (`uploaded`): launches the band's kernels behind its upload event and sends the piece before it — coded
        // while this band travelled — back over the other direction of the link.
        struct Progress { // bands uploaded so far, handed from the uploading thread to the helper
            std::mutex m;
            std::condition_variable cv;
            uint32_t n = 0;
            void set(uint32_t v) { { std::lock_guard<std::mutex> lock(m); if (v > n) n = v; } cv.notify_all(); }
            void wait_beyond(uint32_t k) { std::unique_lock<std::mutex> lock(m); cv.wait(lock, [&] { return n > k; }); }
        } uploaded;
        int helper_rc = PIXO_OK;
        std::string helper_error; // (the helper's failures set ITS thread's message: carried over to the caller's below)
        if (!c.helper) c.helper = new CopyHelper;
        const int device = c.device;
        c.helper->start([&, device] {
            (void)hipSetDevice(device);
            auto body = [&]() -> int {
                for (uint32_t k = 0; k < pieces; ++k) {
                    uploaded.wait_beyond(k);
                    int rc = launch_piece(k);
                    if (rc) return rc;
                    if (k) {
                        HIP_TRY(hipEventSynchronize(c.piece_done[k - 1]));
                        if ((rc = send_piece(k - 1))) return rc;
                    }
                }
                HIP_TRY(hipEventSynchronize(c.piece_done[pieces - 1]));
                const int rc = send_piece(pieces - 1);
                if (rc) return rc;
                HIP_TRY(hipStreamSynchronize(c.copy_stream));
                return PIXO_OK;
            };
            helper_rc = body();
            if (helper_rc) helper_error = t_error;
        });
        // (whatever happens below, the helper must have finished before this frame's variables go away)
        struct HelperGuard { Context &c; Progress &up; uint32_t n; ~HelperGuard() { up.set(n); c.helper->wait(); } } guard{c, uploaded, pieces};
        const uint32_t unit = (!src->g->gray && src->g->s420) ? 16u : 8u;
        const size_t row_bytes = static_cast<size_t>(src->o->width) * (src->g->gray ? 1 : 3);
        for (uint32_t k = 0; k < pieces; ++k) {
            const size_t r0 = static_cast<size_t>(begin[k] / groups_per_row), r1 = k + 1 == pieces ? ~size_t{0} : static_cast<size_t>(begin[k + 1] / groups_per_row);
            const size_t y0 = std::min<size_t>(src->o->height, r0 * unit), y1 = k + 1 == pieces ? src->o->height : std::min<size_t>(src->o->height, r1 * unit);
            if (y1 > y0)
                HIP_TRY(hipMemcpyAsync(static_cast<uint8_t *>(const_cast<void *>(src->d_px)) + y0 * row_bytes, src->host_px + y0 * row_bytes,
                                       (y1 - y0) * row_bytes, hipMemcpyHostToDevice, c.upload_stream));
            HIP_TRY(hipEventRecord(c.band_up[k], c.upload_stream));
            uploaded.set(k + 1);
        }
        sw.lap("  bands uploaded");
        c.helper->wait();
        if (helper_rc) return helper_rc > 0 ? helper_rc : fail(helper_rc, helper_error); // (pixo_hip_last_error() is per thread)
    } else {
        for (uint32_t k = 0; k < pieces; ++k) {
            const int rc = launch_piece(k);
            if (rc) return rc;
        }
        sw.lap("  pieces enqueued");
        for (; next_out < pieces; ++next_out) {
            HIP_TRY(hipEventSynchronize(c.piece_done[next_out]));
            sw.lap("  piece coded");
            const int rc = send_piece(next_out);
            if (rc) return rc;
        }
        HIP_TRY(hipStreamSynchronize(c.copy_stream));
    }
    sw.lap("  copies done");
    if (gave_up) return scan_retry_multipass(c);
    if (redo) return 1;
    *scan_bytes = done;
    return PIXO_OK;
}

} // namespace pixo_capi
