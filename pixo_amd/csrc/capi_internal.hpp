// capi_internal.hpp — what the translation units behind include/pixo_hip.h share (not installed, not part of the ABI).
//
//   context.cpp      error state, per-device table cache, the thread's Context (stream + grow-only buffers), the pool that
//                    outlives threads, device selection, the debug-switch parser
//   scan_job.cpp     coefficient launches on a context; one pass of the device entropy stage in the steps a band needs
//   baseline_file.cpp  device tuple / pixels -> whole baseline file: runs the route baseline_plan.hpp chooses, finishes the file
//   file_route.cpp   pixels or tuple in, a whole file out, to this destination: encode_file (host twin, progressive, baseline),
//                    the delivery of a FileResult, batches into an arena
//   pieces.cpp       a scan coded in pieces while the file travels (and the context's copy helper thread)
//   host_memory.cpp  blocks for files the caller will own (kept large blocks, the pinned pool), copies into fresh memory
//   progressive.cpp  preset 2: trellis tuple, the seven progressive scans, into a FileDest
//   jpeg_api.cpp     the extern "C" JPEG entry points: check arguments -> context -> encode_file -> deliver
//   bands.cpp        one image over several GPUs: band encoder, splice, pixo_hip_jpeg_encode_multi
//   png_api.cpp      the extern "C" PNG row-filter entry points
//   png_reduce_api.cpp  the extern "C" PNG prepare entry points: png_check_options, reductions (png_reduce.hip), palette ordering, the filter
//   png_encode_api.cpp  the extern "C" zlib / PNG whole-file entry points: prepare, the DEFLATE tail over a segment table (png_deflate.hip), file head and IDAT frames;
//                    the PNG batch entries: segments, sub-batches, the batched tail
//   png_quantize_api.cpp  PNG lossy mode: gate, histogram and median cut on the host, the kernels of png_quantize.hip, the extern "C" quantize entries
//   resize_api.cpp   the extern "C" resize entry points, the Lanczos3 contribution tables; the resize batch entries: plan, sub-batches
//   convert_api.cpp  the extern "C" colour-conversion entry points: layout, checks, plan, sub-batches, the launches of convert.hip
//   png_decode_api.cpp  the extern "C" PNG decode entry points: chunk walk and checks, the host inflate (png_inflate.cpp), the runs of rows,
//                    the launches of png_unfilter.hip; the decode batch entries: two-phase checks, the inflate pool, plan, sub-batches
//   jpeg_decode_host.cpp  JPEG decode on the host (no HIP): the marker walk and its checks, the entropy decoder into the kernel's layout
//   jpeg_decode_api.cpp  the extern "C" JPEG decode entry points: two-phase checks, the entropy decodes on the decode pool, plan,
//                    sub-batches, the launches of jpeg_decode.hip
//   batch_steps.hpp  (a header of the host files only) the steps the batch drivers above share: per-record checks, layout, the
//                    sub-batch cut, the caller's stream, the job fence, the host entries' tail
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pixo_hip.h"
#include "jpeg_entropy.hpp"
#include "jpeg_host.hpp"
#include "jpeg_kernels.hpp"
#include "jpeg_pixels_code.hpp"
#include "jpeg_scan_block.h" // (the table form of the flat walk: built on the host, see upload_scan_tables)
#include "baseline_plan.hpp"
#include "routes.hpp"
#include "png_images_math.h"
#include "jpeg_images.hpp"

namespace pixo_capi {

// ---- errors: negative status + thread-local message equal to pixo::Error's Display string (src/error.rs:50-91) --------
extern thread_local std::string t_error;
int fail(int code, const std::string &msg);
int hip_fail(hipError_t e, const char *what); // pixo::Error::CompressionError(String): "Compression error: {msg}"

#define HIP_TRY(expr)                                                  \
    do {                                                               \
        hipError_t e_ = (expr);                                        \
        if (e_ != hipSuccess) return ::pixo_capi::hip_fail(e_, #expr); \
    } while (0)
// A null pointer where the contract wants an object is a caller bug the Rust API cannot express; the C ABI
// answers it with an error instead of a crash.
#define PIXO_REQUIRE(p) do { if (!(p)) return ::pixo_capi::fail(PIXO_ERR_COMPRESSION, "Compression error: null argument '" #p "'"); } while (0)
// The argument checks every entry shares, each at the place the entry's own order gives it.
inline int checked(const pixo_jpeg_options &o, bool with_data = false, size_t data_len = 0) // validation in the reference's order
{
    std::string msg;
    const int rc = pixo_host::validate(o, with_data, data_len, msg);
    return rc ? fail(rc, msg) : PIXO_OK;
}
inline int batch_in_range(uint32_t batch)
{
    return batch == 0 || batch > 65535 ? fail(PIXO_ERR_COMPRESSION, "Compression error: batch must be 1..65535") : PIXO_OK;
}
// The one home of this string: `needed` also goes to *out_len where the entry promises the size with the refusal.
inline int too_small(size_t needed, size_t *out_len = nullptr)
{
    if (out_len) *out_len = needed;
    return fail(PIXO_ERR_BUFFER_TOO_SMALL, "output buffer too small: need " + std::to_string(needed) + " bytes");
}
// ... and of these three (src/error.rs:50-91), for the entries whose checks are not pixo_host::validate's
inline std::string dims(uint32_t w, uint32_t h) { return std::to_string(w) + "x" + std::to_string(h); }
inline int bad_dimensions(uint32_t w, uint32_t h) { return fail(PIXO_ERR_INVALID_DIMENSIONS, "Invalid image dimensions: " + dims(w, h)); }
inline int too_large(uint32_t w, uint32_t h, uint32_t max)
{
    return fail(PIXO_ERR_IMAGE_TOO_LARGE, "Image " + dims(w, h) + " exceeds maximum dimension " + std::to_string(max));
}
inline int bad_length(size_t expected, size_t got)
{
    return fail(PIXO_ERR_INVALID_DATA_LENGTH, "Invalid pixel data length: expected " + std::to_string(expected) + " bytes, got " + std::to_string(got));
}

// ---- debug switches: ONE environment variable, read once ------------------------------------------------------------
// PIXO_HIP_DEBUG="name[=value],name[=value],..." — A/B experiments and tests only; nothing here changes the bytes of a file.
//   trace              per-phase wall times of the device entropy stage on stderr
//   host_entropy       the host twin of the scan coders instead of the device kernels (jpeg_host.cpp)
//   multipass_entropy  the multi-pass entropy kernels (jpeg_entropy.hip) for every scan instead of the single-pass ones
//   direct_stores      the stuffing kernel stores straight into pinned host memory instead of HBM + copy, for files of every size
//   no_direct_small    ... and never, not even for small files (their default since round 4)
//   one_piece          never code a scan in pieces
//   two_kernel_scan    never use the fused pixel -> bit stream kernel (jpeg_pixels_code.hip): coefficient kernel + scan_code as in rounds 2-4
//   fused_batch        batches through the fused kernel whatever the images' width (the default sends batches of images whose 512-pixel
//                      tiles are at least three quarters full through it, every image a segment: scan_job.cpp pixels_code_usable)
//   piece_groups=n     equal pieces of n groups of 192 blocks instead of 2048
//   piece_medium=n     growing pieces from n groups on instead of 1024, whatever the last file's size
//   piece_schedule=a:b:c   their relative sizes (default 1:3)
//   copy_threads=n     threads that copy finished files above 2 MB into fresh host memory (default 8)
//   spin_budget=n      look-back kernels give up waiting after n polls (default 2^20; tests force the fallback with 0)
//   png_batch_bytes=n  a sub-batch of pixo_hip_png_encode_batch* holds at most n bytes of prepared stream (and at least one image)
//                      instead of 64 MiB: tests reach a sub-batch boundary with small images (the limit of 1024 chunks a sub-batch,
//                      which bounds the scratch, stays)
//   resize_batch_bytes=n  a sub-batch of pixo_hip_resize_batch* holds at most n bytes of Lanczos3 intermediate (and at least one
//                      image) instead of 256 MiB: tests reach a sub-batch boundary with small images
//   resize_images_rows=n  an image of pixo_hip_resize_images* has at most n rows of tiles in a pass instead of 65535 (the single
//                      entry's grid.y limit): tests reach the kernels' row-stride loops with small images.  resize_batch_bytes
//                      cuts those entries' sub-batches too
//   convert_images_tiles=n  an image of pixo_hip_convert* has at most n tiles instead of 65536 and a launch at most 2n instead of
//                      2^31 - 1 (convert_math.h): tests reach the kernels' stride loop and a sub-batch seam with small images
//   jpeg_images_blocks=n  a sub-batch of pixo_hip_jpeg_encode_images* holds at most n blocks of 64 coefficients (and at least one image)
//                      instead of 2^22: tests cross a sub-batch seam with small images
//   decode_batch_bytes=n  a sub-batch of pixo_hip_png_decode_batch* holds at most n bytes of device staging (inflated streams +
//                      reconstructed rows; at least one image) instead of 512 MiB: tests reach a sub-batch boundary with small images
//   no_bands_upload    host pixels are uploaded in one copy instead of MCU-row bands pipelined with the kernels
//   plain_host         no host-memory policy (for embedders that own theirs): pixo_hip_free returns every block to malloc at once
//                      (no blocks kept for the next large file), fresh blocks are plain malloc, no madvise(MADV_HUGEPAGE) on the
//                      caller's or the library's memory.  Costs what profiles/r03_fresh_pages.txt shows for files of 24 MiB and more.
struct DebugSwitches {
    bool trace = false, host_entropy = false, multipass_entropy = false, direct_stores = false, one_piece = false;
    bool piece_medium_forced = false, no_bands_upload = false, plain_host = false, no_direct_small = false, two_kernel_scan = false, fused_batch = false;
    int trellis_form = 0; // 1 / 2: the trellis search on one / on eight lanes per block whatever the image's size (jpeg_trellis.hpp)
    int coef_form = 0; // 1 / 2: the coefficient kernel's scalar / packed form whatever the launch size (jpeg_kernels.hpp)
    bool no_side_stats = false; // preset 2 on small images: statistics on the context's stream, in front of the search (round 4's order)
    // host pixels are uploaded in bands from this many MiB of pixels on (bands_upload_min_mb=n), in bands of about
    // bands_upload_mb=n MiB.  A 4096x4096 RGB image (48 MiB) in six bands of 8 MiB: noise 1.18 -> 1.14 ms into caller storage,
    // but a smooth image 0.99 -> 1.10 ms and the malloc'ing entry 1.43 -> 1.55: not below 96 MiB (profiles/r03_host_bands_probe.txt)
    uint32_t bands_upload_min_mb = 96;
    uint32_t bands_upload_mb = 12;
    uint64_t piece_groups = 2048, piece_medium = 1024;
    std::vector<uint32_t> piece_schedule{1, 3};
    unsigned copy_threads = 8;
    uint32_t spin_budget = 1u << 20;
    uint32_t batch_parts = 0; // (measurements) sub-batches of pixo_hip_jpeg_encode_batch_device_into, 0 = the library's choice
    uint64_t png_batch_bytes = 0; // bytes of prepared stream a sub-batch of the PNG batch entries holds at most, 0 = 64 MiB
    uint64_t resize_batch_bytes = 0; // bytes of Lanczos3 intermediate a sub-batch of the resize batch entries holds at most, 0 = 256 MiB
    uint32_t resize_images_rows = 0; // rows of tiles an image of pixo_hip_resize_images* has at most in a pass, 0 = 65535
    uint32_t convert_images_tiles = 0; // tiles an image of the convert entries has at most, 0 = 65536; a launch then holds at most twice as many
    uint64_t jpeg_images_blocks = 0; // blocks a sub-batch of the JPEG images entries holds at most, 0 = 2^22 (jpeg_images_math.h)
    uint64_t decode_batch_bytes = 0; // bytes of device staging a sub-batch of the PNG decode batch entries holds at most, 0 = 512 MiB
};
const DebugSwitches &debug();

// ---- route record (tests: pixo_hip_debug_routes) ----------------------------------------------------------------------
// (the bits: routes.hpp)
void note_route(uint64_t bits);
uint64_t take_routes(bool clear);
// route::CALLER_RETRY is noted by fail(PIXO_ERR_BUFFER_TOO_SMALL) only inside an entry point that was given storage of its
// own (not a size query: a null output or a capacity of 0).  The entry points with caller storage open one of these.
extern thread_local bool t_caller_storage;
struct CallerStorageScope {
    bool prev;
    explicit CallerStorageScope(bool given) : prev(t_caller_storage) { t_caller_storage = given; }
    ~CallerStorageScope() { t_caller_storage = prev; }
    CallerStorageScope(const CallerStorageScope &) = delete;
    CallerStorageScope &operator=(const CallerStorageScope &) = delete;
};

// ---- per-device table cache: 100 qualities x kDeviceQtFloats floats, uploaded once --------------------------------------
constexpr int kMaxDevices = 64;
int device_tables(int device, const float **out);

// Makes a context's device current for the calling thread for the duration of an entry point and gives
// the caller its own device back afterwards (torch and other HIP users share the thread).
struct DeviceScope {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device); else prev = -1;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

// ---- grow-only buffers ---------------------------------------------------------------------------------------------------
// The library's only grow-only buffer: device memory or pinned host memory, with a growth rule fixed per buffer.  Two rules
// keep the buffers sound:
//   * one purpose per buffer: a buffer holds one kind of thing, so that no use of it can move it under another;
//   * a job reserves everything it needs before it hands any address to a kernel: reserve frees the old memory before it
//     allocates the new, so an address taken before a growing reserve is dangling.
// `known` is what the owner knows about the contents (its meaning is the owner's; 0: nothing).  It is forgotten whenever the
// memory is freed or moves.
struct Buf {
    enum class Mem : uint8_t { Device, Pinned };
    enum class Grow : uint8_t {
        Exact,    // n
        Headroom, // n + n/4: sizes are data dependent
        SegEnds,  // u64 words w = n / 8 -> w + w/4 + 16 words
    };
    void *p = nullptr;
    size_t cap = 0; // bytes
    size_t known = 0;
    Mem mem = Mem::Device;
    Grow grow = Grow::Headroom;

    Buf() = default;
    Buf(Mem m, Grow g) : mem(m), grow(g) {}
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    int reserve(size_t n) { return n <= cap ? PIXO_OK : regrow(n); } // a library status (hip_fail)
    void drop();                                                      // back to the driver (on the current device)
    template <class T> T *as() const { return static_cast<T *>(p); }

private:
    int regrow(size_t n);
};

// ---- thread-local execution context --------------------------------------------------
// (every Buf member is listed once, in context.cpp each_buf: held_bytes, shrink_to and release walk that list)
struct Context {
    int device = 0;
    bool ready = false;
    hipStream_t stream = nullptr;
    hipEvent_t producer_done = nullptr; // orders the context's stream after the caller's (device-pointer entries)
    hipEvent_t stats_done = nullptr;    // preset 2: the symbol counts of the statistics pass have reached the host (progressive.cpp)
    hipEvent_t side_ready = nullptr;    // preset 2, small images: the second stream may start (the pixels are there)
    Buf d_px{Buf::Mem::Device, Buf::Grow::Exact};   // pixels uploaded from the host (callers round up to 16 bytes)
    Buf d_coef{Buf::Mem::Device, Buf::Grow::Exact}; // the coefficient tuple
    Buf h_coef{Buf::Mem::Pinned, Buf::Grow::Exact}; // ... copied to the host
    // device entropy stage
    Buf e_tables;                    // known: 1 = it holds tables_held, uploaded on tables_stream (no upload when unchanged)
    Buf e_hist, e_count, e_len, e_off, e_tmp, e_totals, e_stream, e_tile_ff, e_tile_base, e_out, e_seg_bytes, e_seg_off;
    Buf e_code_state, e_stuff_state; // single-pass kernels (jpeg_scan_fused.hip): look-back descriptors, totals.  e_code_state.known: this
                                     //   many of its words are zero (the stuffing kernel cleans up behind itself)
    Buf e_pc_state;                  // the fused pixel -> scan kernel (jpeg_pixels_code.hip): TWO state blocks that alternate — a launch zeroes the
                                     //   block of the launch before it.  known: words per block (both are zero or being zeroed; 0: nothing known)
    int pc_flip = 0;                 //   which block the next launch uses
    Buf e_pc_spill;                  //   where a group of several 6 KiB rounds parks its quantised blocks between the rounds' walks (a buffer of its
                                     //   own: growing d_coef here would free the tuple a caller's retry path still points into)
    Buf e_chain;                     // a scan coded in pieces: bits / bytes of the scan before every piece (device_entropy_pieces)
    Buf e_seams;                     // batch files that stay in HBM: their offsets + the header bytes for batch_seams_kernel
    Buf e_segs;                      // segmented scans (batches, restart intervals): per-segment results of the single-pass kernels
    Buf h_segs{Buf::Mem::Pinned, Buf::Grow::SegEnds}; // u64 words: where every segment of a segmented scan ends (reserved by scan_begin)
    hipStream_t copy_stream = nullptr; // ... whose bytes travel to the host on this stream while the next piece is coded
    hipStream_t upload_stream = nullptr; // host pixels arrive band by band on this stream while earlier bands are transformed
    struct CopyHelper *helper = nullptr; // ... and a second host thread sends the coded pieces back meanwhile (pieces.cpp; stopped and joined by release())
    std::vector<hipEvent_t> piece_done, band_up;
    uint32_t tables_held[pixo_scan::kScanTableUpload]; hipStream_t tables_stream = nullptr; // what e_tables holds
    uint64_t last_prog_bytes = 0; // the last progressive file's entropy-coded bytes (small: the next one is stored directly)
    // the last whole baseline scan this context coded (0 blocks: none yet; baseline_file.cpp remember_scan): predicts the next
    // file's size and density (baseline_plan.hpp).  Exact: a smooth image is below one byte per block
    uint64_t last_scan_bytes = 0, last_scan_blocks = 0;
    uint32_t batch_per_block = 0;  // ... of the last batch (1 + bytes per block; 0: none yet): whether sub-batches pay, jpeg_api.cpp
    Buf p_in, p_out, p_sums, p_scratch; // PNG filter stage
    Buf h_sums{Buf::Mem::Pinned, Buf::Grow::Exact}; // ... p_sums copied to the host
    Buf p_images, h_images{Buf::Mem::Pinned, Buf::Grow::Exact}; // the records of a ragged filter launch (png_images_math.h) and what they go up from
    Buf j_tables, h_jtables{Buf::Mem::Pinned, Buf::Grow::Headroom}; // JPEG images (jpeg_images_api.cpp): a sub-batch's tile and segment records and what they go up from
    Buf j_out;                       // ... the stuffed scans of its RGB pass (the gray pass's lie in e_out) until both have been delivered
    // PNG reductions (png_reduce_api.cpp)
    Buf q_work{Buf::Mem::Device, Buf::Grow::Exact};  // one PngWork: analysis, key lookup table, index map, histogram, pair counts
    Buf h_qwork{Buf::Mem::Pinned, Buf::Grow::Exact}; // ... its host side: results come down into it, tables go up from it
    Buf q_index{Buf::Mem::Device, Buf::Grow::Exact}; // palette case: the index image (sorted-key order), 1 byte per pixel
    Buf q_rows{Buf::Mem::Device, Buf::Grow::Exact};  // the reduced rows the filter kernel reads
    // device DEFLATE (png_encode_api.cpp, png_deflate.hip)
    Buf z_tok{Buf::Mem::Device, Buf::Grow::Exact};   // a token per input byte, 65,536 u32 per chunk
    Buf z_slots{Buf::Mem::Device, Buf::Grow::Exact}; // a slot per chunk: its block before compaction
    Buf z_prev{Buf::Mem::Device, Buf::Grow::Exact};  // high effort only: a u16 link per position of every chunk and of its window
    Buf z_info;                                      // per chunk: block bytes, form, Adler sums; behind them the blocks' offsets (u64)
    Buf z_stream;                                    // the zlib stream: plain, or as IDAT bodies with room for their frames
    Buf z_crc;                                       // CRC-32 of every 4 KiB piece of the stream
    Buf h_zinfo{Buf::Mem::Pinned, Buf::Grow::Headroom}; // ... z_info / z_crc copied to the host
    // PNG quantisation (png_quantize_api.cpp, png_quantize.hip); the indices go to q_index
    Buf k_samples{Buf::Mem::Device, Buf::Grow::Exact};  // the strided colour keys of the histogram and of the gate
    Buf h_ksamples{Buf::Mem::Pinned, Buf::Grow::Exact}; // ... copied to the host (and sorted there)
    Buf k_work{Buf::Mem::Device, Buf::Grow::Exact};     // one QuantWork: histogram colours and counts, palette, k-means sums, dither state
    Buf h_kwork{Buf::Mem::Pinned, Buf::Grow::Exact};    // ... its host side
    Buf k_lut{Buf::Mem::Device, Buf::Grow::Exact};      // the 64^3 nearest-entry table
    Buf k_carry{Buf::Mem::Device, Buf::Grow::Exact};    // dither: per band, what its first row receives from the band above (u64 per column)
    Buf t_raw, t_trail;                 // progressive + trellis: unquantised DCT blocks (f32), Viterbi back-pointers
    Buf t_plain;                        // preset 2, small images: the plain quantiser's tuple of the statistics pass on the second stream
    Buf g_flags, g_rank, g_by_rank;     // progressive scans: band flags, rank among non-empty blocks and its inverse
    Buf h_file{Buf::Mem::Pinned, Buf::Grow::Headroom}; // the finished file lands here
    // resize (resize_api.cpp)
    Buf r_in{Buf::Mem::Device, Buf::Grow::Exact}, r_out{Buf::Mem::Device, Buf::Grow::Exact}; // host entries: pixels up, resized pixels down
    Buf r_mid;                                          // Lanczos3: the u8 intermediate between the passes (src_h rows, padded)
    Buf r_tables;                                       // ... both axes' contribution tables; known: 1 = they are those of r_dims
    Buf r_stage{Buf::Mem::Pinned, Buf::Grow::Headroom}; // ... built here on the host, uploaded from here
    uint32_t r_dims[4] = {0, 0, 0, 0};                  // src_w, dst_w, src_h, dst_h of the tables held
    uint32_t r_max_span = 0;                            // ... the widest source span of one horizontal tile
    size_t r_v_at = 0;                                  // ... where the vertical axis starts in r_tables
    hipEvent_t r_done = nullptr;                        // the last Lanczos3 job (it reads r_tables, writes r_mid) has run
    // resize batches (resize_api.cpp): buffers of their own, so that the single entry's cached tables stay what r_dims says
    Buf rb_in{Buf::Mem::Device, Buf::Grow::Exact}, rb_out{Buf::Mem::Device, Buf::Grow::Exact}; // host entry: every source up, the block of images down
    Buf rb_mid;                                          // Lanczos3: the intermediates of one sub-batch, image after image
    Buf rb_tables;                                       // the axis tables of a call, behind them its ResizeBatchItem per image
    Buf rb_stage{Buf::Mem::Pinned, Buf::Grow::Headroom}; // ... built here on the host, uploaded from here in one copy
    hipEvent_t rb_done = nullptr;                        // the last batch job (it reads rb_tables, writes rb_mid) has run
    // colour conversion (convert_api.cpp, convert.hip)
    Buf cv_in{Buf::Mem::Device, Buf::Grow::Exact}, cv_out{Buf::Mem::Device, Buf::Grow::Exact}; // host entries: the block of sources up, the block of destinations down
    Buf cv_records;                                        // the records of a call's launches (convert_math.h), sub-batch after sub-batch
    Buf h_cv_records{Buf::Mem::Pinned, Buf::Grow::Headroom}; // ... built here on the host, uploaded from here, one copy per sub-batch
    hipEvent_t cv_done = nullptr;                          // the last convert job (it reads cv_records) has run
    // PNG decode (png_decode_api.cpp, png_unfilter.hip)
    Buf u_inflated{Buf::Mem::Pinned, Buf::Grow::Exact};  // the inflated stream (a batch: all its streams): the host inflate writes it, the upload reads it
    Buf u_stream{Buf::Mem::Device, Buf::Grow::Exact};    // ... on the device
    Buf u_rows{Buf::Mem::Device, Buf::Grow::Exact};      // the reconstructed rows, 16-byte pitched
    Buf u_out{Buf::Mem::Device, Buf::Grow::Exact};       // host entry: the pixels before they go down
    Buf u_tables{Buf::Mem::Device, Buf::Grow::Exact};    // the palette table (256 words), behind it the runs of rows (a batch: descriptions, runs, block tables, palettes)
    Buf h_utables{Buf::Mem::Pinned, Buf::Grow::Headroom}; // ... built here, uploaded from here
    // ... batches with PIXO_DECODE_DEVICE_INFLATE (png_inflate.hip): per sub-batch
    Buf h_zin{Buf::Mem::Pinned, Buf::Grow::Headroom};    // the stream and gather descriptions, behind them the compressed streams, each padded
    Buf u_zin{Buf::Mem::Device, Buf::Grow::Exact};       // ... on the device
    Buf u_zout{Buf::Mem::Device, Buf::Grow::Exact};      // the status record of every stream, behind them every image's filter bytes
    Buf h_zout{Buf::Mem::Pinned, Buf::Grow::Headroom};   // ... copied to the host
    Buf h_uruns{Buf::Mem::Pinned, Buf::Grow::Headroom};  // a sub-batch's runs of rows, which are known only behind its inflate
    Buf u_runs{Buf::Mem::Device, Buf::Grow::Exact};      // ... on the device
    hipEvent_t u_done = nullptr;                         // the last decode job (it reads all of the above) has run
    // JPEG decode (jpeg_decode_api.cpp, jpeg_decode.hip)
    Buf jd_hcoef{Buf::Mem::Pinned, Buf::Grow::Exact};    // a call's quantised coefficients in the kernel's layout: the entropy decoders write them, the uploads read them
    Buf jd_coef{Buf::Mem::Device, Buf::Grow::Exact};     // ... one sub-batch's on the device
    Buf jd_hrecords{Buf::Mem::Pinned, Buf::Grow::Headroom}; // the records of a call's launches (jpeg_decode_math.h), built here, uploaded from here
    Buf jd_records{Buf::Mem::Device, Buf::Grow::Exact};  // ... on the device
    Buf jd_out{Buf::Mem::Device, Buf::Grow::Exact};      // host entries: the pixels before they go down
    Buf jd_hscan{Buf::Mem::Pinned, Buf::Grow::Headroom};  // PIXO_DECODE_DEVICE_ENTROPY: a sub-batch's file records (jpeg_entropy_dec_math.h) and raw scans, built here, uploaded from here
    Buf jd_scan{Buf::Mem::Device, Buf::Grow::Exact};     // ... on the device
    Buf jd_states{Buf::Mem::Device, Buf::Grow::Headroom}; // ... the lanes' states, block counts and first blocks, the workgroups' border states
    Buf jd_estatus{Buf::Mem::Device, Buf::Grow::Headroom}; // ... the launches' counters and the files' status records
    Buf jd_hestatus{Buf::Mem::Pinned, Buf::Grow::Headroom}; // ... copied to the host
    hipEvent_t jd_done = nullptr;                        // the last JPEG decode job (it reads all of the above) has run

    // Small results for the host, one field per purpose: pinned, allocated once with the stream (ensure).
    struct Mailbox {
        static constexpr size_t kTotalsWords = 4 * 32;
        uint64_t totals[kTotalsWords];                 // the kernels' totals, 4 words per piece of a scan: [0] bits, [1] stuffed bytes,
                                                       //   [2] packed bytes or tiles, [3] a look-back gave up
        uint64_t counts[pixo_host::kScanTableWords];   // symbol counts of an optimised-tables pass
        int16_t last_dc[4];                            // the band encoder: last DC of every plane
        uint32_t tables[pixo_scan::kScanTableUpload];  // staging of upload_scan_tables
    };
    Mailbox *mail = nullptr;

    int ensure();
    size_t held_bytes() const; // device + pinned bytes this context keeps
    void shrink_to(size_t max_buffer_bytes); // releases every buffer larger than this (a parked context keeps the small ones)
    void release(); // everything back to the driver; the context starts over at its next use
};
// The totals as the kernels take them
inline unsigned long long *mailbox(Context &c) { return reinterpret_cast<unsigned long long *>(c.mail->totals); }

// ---- small facts of an image, said once ----------------------------------------------------------------------------------
inline pixo_host::Geometry geometry_of(const pixo_jpeg_options &o) { return pixo_host::geometry(o.width, o.height, o.color_type, o.subsampling); }
inline size_t pixel_bytes(const pixo_jpeg_options &o, const pixo_host::Geometry &g) { return static_cast<size_t>(o.width) * o.height * (g.gray ? 1 : 3); }
inline uint32_t bytes_per_pixel(uint8_t color_type) { return color_type + 1u; } // PIXO_GRAY 1, PIXO_GRAY_ALPHA 2, PIXO_RGB 3, PIXO_RGBA 4
inline int reserve16(Buf &b, size_t n) { return b.reserve((n + 15) & ~size_t{15}); } // what kernels read as pixels: they load 16 bytes at a time
inline int reserve_pixels(Context &c, size_t n) { return reserve16(c.d_px, n); }
inline int upload(Context &c, Buf &b, const void *host, size_t n) // host bytes into `b`, on the context's stream
{
    if (const int rc = reserve16(b, n)) return rc;
    HIP_TRY(hipMemcpyAsync(b.p, host, n, hipMemcpyHostToDevice, c.stream));
    return PIXO_OK;
}
// The planes of a tuple that lies in one buffer: Y of every image of the batch, then Cb, then Cr (64 coefficients per block).
template <class T> struct PlanesOf { T *y, *cb, *cr; };
using Planes = PlanesOf<int16_t>;
template <class T> PlanesOf<T> planes_of(T *base, const pixo_host::Geometry &g, size_t batch = 1)
{
    T *cb = base + g.y_blocks * 64 * batch;
    return {base, cb, cb + g.c_blocks * 64 * batch};
}

// Contexts outlive the threads that use them (context.cpp): a thread that ends parks its context in the pool — no HIP
// call in a thread-local destructor — and the next thread that needs one adopts it.
struct ContextPool {
    std::mutex m;
    std::vector<Context *> idle;
    Context *take(int device);
    void give(Context *c); // no HIP calls: may run in a thread-local destructor
    void drain();          // frees every parked context (pixo_hip_trim)
};
ContextPool &pool();
struct ThreadSlot {
    Context *c = nullptr;
    int device = 0; // pixo_hip_set_device
    ~ThreadSlot();
};
extern thread_local ThreadSlot t_slot;
Context &thread_context();

#define PIXO_ON_DEVICE_OF(ctx)                                    \
    ::pixo_capi::DeviceScope device_scope_((ctx).device);         \
    if (device_scope_.err != hipSuccess) return ::pixo_capi::hip_fail(device_scope_.err, "hipSetDevice")
// The preamble of an entry point that works on the thread's own context: declares it as `c`, ready, its device current
#define PIXO_THREAD_CONTEXT(c)                                \
    ::pixo_capi::Context &c = ::pixo_capi::thread_context();  \
    if (const int ensure_rc_ = c.ensure()) return ensure_rc_; \
    PIXO_ON_DEVICE_OF(c)

// Device-pointer entry points run on the context's own stream.  What the caller enqueued before the call — on the stream
// it named with pixo_hip_set_producer_stream, by default the NULL stream — is ordered in front of it with an event.
int order_after_producer(Context &c);
int context_on_current_device(Context **out); // binds the thread's context to the HIP device that is current for the caller

struct Stopwatch { // debug switch `trace`: per-phase wall times of the device entropy stage on stderr
    bool on = debug().trace;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char *what)
    {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[pixo_hip] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

void destroy_copy_helper(struct CopyHelper *h); // pieces.cpp (the type is complete only there)

// What the runtime knows of a host or device address.  Plain malloc'd memory is "invalid value" to it: not an error — the
// lookup's error is cleared and the type stays hipMemoryTypeUnregistered.  Each caller decides which types it accepts.
struct PointerInfo {
    hipMemoryType type = hipMemoryTypeUnregistered;
    int device = -1;
    void *device_ptr = nullptr; // (pinned / registered host memory: the address the GPU stores to)
};
inline PointerInfo pointer_info(const void *p)
{
    PointerInfo r;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return r; }
    r.type = at.type;
    r.device = at.device;
    r.device_ptr = at.devicePointer;
    return r;
}

// ---- host memory helpers (host_memory.cpp) --------------------------------------------------------------------------
template <class F> void run_on_threads(unsigned t, F &&body) // body(index) for index in [0, t)
{
    if (t <= 1) { body(0u); return; }
    std::vector<std::thread> workers;
    workers.reserve(t - 1);
    for (unsigned i = 1; i < t; ++i) workers.emplace_back([&body, i] { body(i); });
    body(0u);
    for (auto &w : workers) w.join();
}
void big_copy(uint8_t *dst, const uint8_t *src, size_t n);
void advise_huge(void *p, size_t n);
uint8_t *alloc_file(size_t n); // a block for a finished file that the caller will own: large ones come from the blocks pixo_hip_free kept
void free_file(void *p);       // pixo_hip_free: large blocks are kept (at most two) for the next large file
void drop_kept_blocks();       // pixo_hip_trim
void drop_batch_worker_buffers(); // pixo_hip_trim: the device buffers of pixo_hip_jpeg_encode_batch_multi's worker threads (bands.cpp)
uint8_t *pool_take(size_t n);  // a block of PINNED host memory for a file the caller will own (null: none to be had — malloc instead); back via free_file
int deliver(const uint8_t *file, size_t n, uint8_t **out, size_t *out_len);   // a fresh malloc block the caller owns
int hand_over(const std::vector<uint8_t> &v, uint8_t **out, size_t *out_len);

// ---- coefficient launches on a context (scan_job.cpp) -----------------------------------------------------------------
int coeffs_to_pinned(Context &c, const uint8_t *pixels, const pixo_jpeg_options &o, const pixo_host::Geometry &g,
                     const int16_t **y, const int16_t **cb, const int16_t **cr);
int coeffs_reserve(Context &c, const pixo_host::Geometry &g, int16_t **dy, int16_t **dcb, int16_t **dcr);
int coeffs_rows(Context &c, const void *d_pixels, const pixo_jpeg_options &o, const pixo_host::Geometry &g, hipStream_t stream,
                int16_t *dy, int16_t *dcb, int16_t *dcr, uint32_t row0, uint32_t rows);
int coeffs_on_device(Context &c, const void *d_pixels, const pixo_jpeg_options &o, const pixo_host::Geometry &g, hipStream_t stream,
                     int16_t **dy, int16_t **dcb, int16_t **dcr);
bool scan_has_restart_markers(const pixo_jpeg_options &o, const pixo_host::Geometry &g);
// The arguments of a statistics walk over a whole image's tuple (optimised tables: no tables yet, predictors from zero)
inline pixo_dev::ScanArgs count_args(const pixo_host::Geometry &g, const pixo_jpeg_options &o, const int16_t *dy, const int16_t *dcb, const int16_t *dcr)
{
    pixo_dev::ScanArgs a;
    a.y = dy; a.cb = dcb; a.cr = dcr; a.tables = nullptr;
    a.mode = g.gray ? 0 : (g.s420 ? 2 : 1);
    a.nblocks = g.y_blocks + 2 * g.c_blocks;
    a.blocks_per_mcu = g.gray ? 1 : (g.s420 ? 6 : 3);
    a.marker_bytes = 2;
    a.restart = scan_has_restart_markers(o, g) ? o.restart_interval : 0;
    a.seed_dc[0] = a.seed_dc[1] = a.seed_dc[2] = 0; a.bit_base = 0; a.pad_last = 1;
    return a;
}

// ---- the device entropy stage, in the steps a caller may need to interleave with exchanges (scan_job.cpp) ------------
// One pass over a coefficient tuple in HBM: a whole image, a batch of images (one byte-aligned segment each), or a
// BAND of a larger image (predictors seeded from the band above, packed at the band's bit offset modulo 8,
// no final padding).
struct ScanJob {
    const void *count_px = nullptr; // optimised tables of a scan the fused kernel codes: the statistics come from these device pixels (scan_tables)
    pixo_dev::ScanArgs a;
    uint64_t n = 0, nseg = 0;
    size_t tmp_blocks = 0, tmp_segs = 0, tmp_tiles = 0;
    pixo_dev::SegmentPlan plan{0, nullptr};
    pixo_host::HuffSet h;
    uint64_t total_bits = 0;
    uint64_t nbytes = 0;     // bytes of the packed stream that get stuffed (a band: its whole bytes only)
    uint64_t scan_bytes = 0; // ... after stuffing, in c.e_out
    bool band = false;
    bool tables_ready = false; // j.h is built and on the device (scan_tables)
    int head_bits = 0;       // band: how many of its first bits share a byte with the band before
    bool fused = false;      // one uninterrupted scan: the two single-pass kernels of jpeg_scan_fused.hip
    bool segmented = false;  // byte-aligned segments (images of a batch, restart intervals) in the single-pass kernels
    bool pc_seg = false;     // ... coded as segments of the fused pixel -> scan kernel (scan_from_pixels): c.h_segs, seg.marker_bytes as for `segmented`
    pixo_dev::SegArgs seg;   // ... their geometry and per-segment arrays (c.e_segs, c.h_segs)
    uint32_t seg_gap = 0;    // set BEFORE scan_begin: bytes a batch wants left free between its images' scans in c.e_out
                             // (headers + EOI: the whole batch then leaves the device in one copy); honoured only by segmented jobs
    size_t stream_cap = 0;   // fused: bytes the packed stream can take at most
    size_t code_state_words = 0; // fused: u64 words of c.e_code_state the code kernel of this job uses (the stuffing kernel zeroes them again)
};
// A step of a job returns this when a single-pass kernel gave up waiting (bounded look-back, jpeg_scan_fused.hip): nothing of
// the job's results is valid; run the job again inside a RetryMultipass scope, which makes scan_begin choose the multi-pass
// kernels.  (Internal: never returned through the C ABI.)
constexpr int kRetryMultipass = 1000;
extern thread_local bool t_force_multipass;
struct RetryMultipass {
    RetryMultipass() { t_force_multipass = true; }
    ~RetryMultipass() { t_force_multipass = false; }
};
int scan_retry_multipass(Context &c);
uint64_t lookback_fallbacks(); // how often that has happened in this process (tests)
void note_lookback_fallback();  // a kernel with bounded waits gave up and its job ran again in a form that waits for nothing (also: the PNG dither)
int upload_scan_tables(Context &c, const uint32_t (&packed)[pixo_host::kScanTableWords], hipStream_t stream);
int scan_begin(Context &c, ScanJob &j, const int16_t *dy, const int16_t *dcb, const int16_t *dcr, const pixo_jpeg_options &o,
               const pixo_host::Geometry &g, uint32_t batch, const int16_t *band_seed_dc);
void split_counts(const uint64_t counts[pixo_host::kScanTableWords], uint64_t dc[2][12], uint64_t ac[2][256]);
int scan_count(Context &c, ScanJob &j, hipStream_t stream, uint64_t counts[pixo_host::kScanTableWords]);
int scan_tables(Context &c, ScanJob &j, const pixo_jpeg_options &o, const pixo_host::Geometry &g, hipStream_t stream, const uint64_t *counts);
int scan_lengths(Context &c, ScanJob &j, const pixo_jpeg_options &o, const pixo_host::Geometry &g, hipStream_t stream,
                 const uint64_t *counts, bool wait = true);
// Where the stuffed bytes go when not into the context's device buffer: host memory the GPU can write (pinned), so that
// the kernel's stores ARE the transfer — no second pass over the file, no second synchronisation.
struct HostTarget {
    uint8_t *p = nullptr; // device-visible address of the first stuffed byte
    size_t cap = 0;       // bytes available from there
    bool grow = false;    // p lies in the context's own pinned file buffer: too small = reserve more and repeat
    size_t before = 0, after = 0; // (grow) bytes the file needs in front of / behind the stuffed bytes
};
// The fused pixel -> bit stream kernel (jpeg_pixels_code.hip) in place of coefficient kernel + scan_code for this job?  (one
// RGB image, one uninterrupted scan, tables known without the tuple's statistics)
bool pixels_code_usable(const ScanJob &j, const pixo_jpeg_options &o, const pixo_host::Geometry &g, uint32_t batch);
// ... tables + that kernel: afterwards the finished (stuffed, padded) scan lies in c.e_out — or at `host`, memory of the host
// that the GPU can write — and j.scan_bytes / j.total_bits / j.nbytes say how long it is.  No tuple, no packed stream is written.
// wait = false: only enqueued (measurements); the totals are then in c.mail->totals[0..2] once the stream has been synchronised.
int scan_from_pixels(Context &c, ScanJob &j, const pixo_jpeg_options &o, const pixo_host::Geometry &g, hipStream_t stream, const void *d_pixels,
                     HostTarget *host, bool wait = true, uint32_t batch = 1);
int scan_stuff_fused(Context &c, ScanJob &j, hipStream_t stream, uint64_t band_bit_offset, uint32_t *head, int *tail_bits,
                     uint32_t *tail, bool chained = false, HostTarget *host = nullptr);
int scan_pack(Context &c, ScanJob &j, hipStream_t stream, uint64_t band_bit_offset = 0, uint32_t *head = nullptr,
              int *tail_bits = nullptr, uint32_t *tail = nullptr);

// ---- whole baseline files (baseline_file.cpp; the route: baseline_plan.hpp) ------------------------------------------
// Pixels whose coefficients have not been computed yet (the tuple's place is reserved): the entropy stage launches the
// coefficient kernel itself — for a scan coded in pieces, band by band in front of each piece.  host_px != null: the
// pixels are still in HOST memory and are uploaded band by band as well (upload_stream), each band's kernels waiting
// only for its own rows.
struct PixelSource {
    const void *d_px;
    const pixo_jpeg_options *o;
    const pixo_host::Geometry *g;
    int16_t *dy, *dcb, *dcr;
    const uint8_t *host_px = nullptr;
};
// Where encode_baseline_file puts the file.  Pinned by default on purpose: a device-to-host copy into fresh pageable memory
// makes the runtime pin those pages first, which costs 10-25 ms for an 11 MB file every time the address changes.
struct FileDest {
    DestKind kind = DestKind::Pinned;
    uint8_t *p = nullptr; size_t cap = 0; // Caller: the file goes straight into this storage (no pinned intermediate); when it
                                          // does not fit, nothing is copied there and the result's len says how much is needed
    uint32_t batch = 1, seg_gap = 0;      // InHbm: `batch` (2 or more) equal images back to back, every one a byte-aligned
                                          // segment of ONE scan; seg_gap: bytes to leave free in c.e_out between their scans
    // (a null `p` is a size query: nothing is stored, the result's len says how much is needed)
    static FileDest caller(uint8_t *p, size_t cap)
    {
        static uint8_t nowhere;
        FileDest d; d.kind = DestKind::Caller; d.p = p ? p : &nowhere; d.cap = p ? cap : 0; return d;
    }
    // OwnBlock: once the size is known the block is allocated and the device-to-host copy goes straight into it; the copy into
    // pageable memory runs at the link's rate, and what it saves is the second pass over the file from the pinned buffer
    // (tools/ubench/upload.cpp: 0.21 ms + a warm 11 MB memcpy, or 1.30 against 1.38 ms for new pages).  Pieces and direct
    // stores fill the pinned buffer instead (the result's own_block stays false): the caller copies with deliver.
    static FileDest own_block() { FileDest d; d.kind = DestKind::OwnBlock; return d; }
    static FileDest in_hbm(uint32_t batch, uint32_t seg_gap) { FileDest d; d.kind = DestKind::InHbm; d.batch = batch; d.seg_gap = seg_gap; return d; }
};
struct FileResult {
    const uint8_t *file = nullptr; // the whole file (InHbm: null)
    size_t len = 0;                // its bytes; InHbm: the bytes of the stuffed scans in c.e_out; PIXO_ERR_BUFFER_TOO_SMALL: the size needed
    size_t header_len = 0;
    bool own_block = false;        // `file` is a block the caller owns (OwnBlock, copied-out route)
    std::vector<uint8_t> head;     // InHbm: the file headers, the same for every image (no EOI is written)
    // InHbm: where each image's bytes begin in c.e_out (batch + 1 entries).  gaps_left: seg_gap was left between the images'
    // scans — only segmented single-pass jobs can —; image_starts then counts the gaps, image i's bytes are
    // [starts[i], starts[i + 1] - gap).
    std::vector<uint64_t> image_starts;
    bool gaps_left = false;
    bool tuple_done = false;       // the tuple has been computed (a multi-pass retry does not compute it again)
    std::vector<uint8_t> spill;    // the host twin's file (debug switch host_entropy): `file` points into it
};
// The tuple dy / dcb / dcr has been computed (src null), or its place is reserved for src's pixels.
int encode_baseline_file(Context &c, const int16_t *dy, const int16_t *dcb, const int16_t *dcr, const PixelSource *src,
                         const pixo_jpeg_options &o, const pixo_host::Geometry &g, const FileDest &dest, FileResult &res);
// A scan coded in pieces while the file travels (pieces.cpp): 0 = its *scan_bytes are at dst; 1 = it outgrew its guesses and
// nothing of it is kept (code it again in one piece); kRetryMultipass; or an error.
int device_entropy_pieces(Context &c, ScanJob &j, hipStream_t stream, uint8_t *dst, size_t dst_cap, uint64_t *scan_bytes,
                          const PixelSource *src);

// ---- pixels or tuple in, a whole file out, to this destination (file_route.cpp) ------------------------------------------
struct FileSource { // what the file is made from: exactly one of the three
    const uint8_t *host_px = nullptr;                           // host pixels (uploaded by the route), or
    const void *d_px = nullptr;                                 // device pixels, or
    const int16_t *dy = nullptr, *dcb = nullptr, *dcr = nullptr; // a device tuple already computed
    static FileSource host(const uint8_t *px) { FileSource s; s.host_px = px; return s; }
    static FileSource device(const void *px) { FileSource s; s.d_px = px; return s; }
    static FileSource tuple(const void *y, const void *cb, const void *cr) { FileSource s; s.dy = static_cast<const int16_t *>(y); s.dcb = static_cast<const int16_t *>(cb); s.dcr = static_cast<const int16_t *>(cr); return s; }
};
// The only place that chooses between the host twin (debug switch host_entropy), the progressive file and the baseline file.
// `c` is ready, its device current, its stream ordered behind the source's producer.
int encode_file(Context &c, const FileSource &src, const pixo_jpeg_options &o, const pixo_host::Geometry &g, const FileDest &dest,
                FileResult &res);
// A FileResult into what the entry promised.  own_block destinations: a block the caller releases with pixo_hip_free.
int deliver_block(FileResult &r, uint8_t **out, size_t *out_len);
// Caller storage, after encode_file returned rc: *out_len (also with PIXO_ERR_BUFFER_TOO_SMALL), then the file unless it
// already lies in `output`.  copy_threads: the library's copy threads for large files (big_copy) instead of one memcpy.
int deliver_into(int rc, const FileResult &r, uint8_t *output, size_t capacity, size_t *out_len, bool copy_threads);
int encode_to_block(Context &c, const FileSource &src, const pixo_jpeg_options &o, const pixo_host::Geometry &g, uint8_t **out,
                    size_t *out_len); // encode_file to own_block, delivered
int encode_host_pixels(const uint8_t *data, const pixo_jpeg_options &o, const FileDest &dest, FileResult &res); // encode_file on the thread's context
// `batch` images back to back in `arena` (host memory of any kind, device memory, or null: sizes only)
int encode_batch_into(Context &c, const void *d_pixels, const pixo_jpeg_options &o, const pixo_host::Geometry &g, uint32_t batch,
                      uint8_t *arena, size_t capacity, size_t *offsets, size_t *lens);
int encode_batch_blocks(Context &c, const void *d_pixels, const pixo_jpeg_options &o, const pixo_host::Geometry &g, uint32_t batch,
                        uint8_t **files, size_t *lens);

// ---- PNG (png_api.cpp) -----------------------------------------------------------------------------------------------
// Argument checks shared by the PNG entries; resolves the strategy the reference would run.  `area` is the image's PIXEL count:
// rows of packed samples are filtered as width = row bytes, bpp = 1, but the small-image rule counts pixels.
int png_plan(uint32_t width, uint32_t height, uint64_t area, uint32_t bpp, uint8_t strategy, uint32_t flags, int *run, bool *sequential_fast);
// filter kernel + checksum on the context's stream; returns after the checksum has been combined
int png_filter_on_device(Context &c, const void *d_in, uint32_t width, uint32_t height, uint32_t bpp, int run, bool sequential_fast,
                         void *d_out, uint32_t *adler);
// `batch` equal images back to back at d_in in one launch, their streams back to back at d_out; the row sums are on their way
// to the host when this returns.  Once the stream has been synchronised, png_filter_batch_adler combines image i's.
int png_filter_batch_begin(Context &c, const void *d_in, uint32_t width, uint32_t height, uint32_t batch, uint32_t bpp, int run, void *d_out);
// ... the Adler-32 of one image from its own rows' sums: `height` rows of row_bytes + 1 stream bytes, the first row's sums at
// index sums_at of the sums that came down (equal images: image * height)
uint32_t png_filter_batch_adler(const Context &c, uint64_t sums_at, uint32_t height, uint64_t row_bytes);
// Images of individual sizes (png_images_math.h): the items' records go up in one copy, one launch per class of images
// present, all row sums on their way down in one copy; item k's sums start at the heights in front of it summed.  Nothing is
// waited for.  *launches: how many filter launches were made.
int png_filter_images_begin(Context &c, const void *d_in, const std::vector<pixo_png_images::Item> &items, void *d_out, uint32_t *launches);

// ---- PNG prepare (png_reduce_api.cpp) --------------------------------------------------------------------------------
// The prepare and whole-file entries' checks in the reference's order; with_data: the host pixels' length too (one that passes IS the input size)
// images: the data are those of a batch of so many equal images back to back
int png_check_options(const pixo_png_options *o, bool with_data = false, size_t data_len = 0, uint32_t images = 1);
// ... its first three: a zero side, a side above the reference's limit, a colour type that is none of the four
int png_check_image(uint32_t width, uint32_t height, uint8_t color_type);
// How the filters saw the rows (packed and palette rows: as one-byte pixels): what a match search behind them is told.
struct PngFilterView { uint32_t bpp, row; }; // bytes per filter pixel, bytes per filtered row
// d_px: width * height * bpp bytes on the context's device; reductions + filters, the stream is left in d_out
int png_prepare_on_device(Context &c, const void *d_px, const pixo_png_options &o, void *d_out, pixo_png_layout *layout, size_t *out_len,
                          uint32_t *adler, PngFilterView *view = nullptr);

// ---- PNG quantisation (png_quantize_api.cpp) ---------------------------------------------------------------------------
// The reference's gate and quantize_image (mod.rs:469-492) on pixels on the context's device.  *applied false: the gate
// declined (or the mode is Off, or the pixels are gray) and nothing else is set.  Otherwise width * height indices lie in
// c.q_index, `layout` describes the 8-bit palette image and *trns_len says how many alphas its tRNS chunk holds (0: none).
int png_check_quantization(const pixo_png_quantization *quantization); // behind png_check_options' checks: a null struct, an unknown mode
int png_quantize_on_device(Context &c, const void *d_px, const pixo_png_options &o, const pixo_png_quantization &q, bool *applied,
                           pixo_png_layout *layout, uint32_t *trns_len);

// ---- preset 2 (progressive.cpp) -----------------------------------------------------------------------------------
int huffman_for_tuple(const int16_t *dy, const int16_t *dcb, const int16_t *dcr, const pixo_jpeg_options &o,
                      const pixo_host::Geometry &g, Context &c, pixo_host::HuffSet &h);
// The file is assembled in caller storage the GPU can write (pinned / registered) when it fits there — res.file == dest.p then —
// and in the context's pinned buffer otherwise: the caller delivers it from there.
int device_progressive_scans(const int16_t *dy, const int16_t *dcb, const int16_t *dcr, const pixo_host::Geometry &g,
                             const pixo_host::HuffSet &h, Context &c, const std::vector<uint8_t> &head, const FileDest &dest, FileResult &res);
// host_twin: the scans are coded by the host twin on a pinned copy of the tuple, into res.spill
int progressive_to_view(const void *d_pixels, const pixo_jpeg_options &o, const pixo_host::Geometry &g, Context &c, bool host_twin,
                        const FileDest &dest, FileResult &res);

} // namespace pixo_capi
