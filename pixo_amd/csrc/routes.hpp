// routes.hpp — the route record's bits (tests: pixo_hip_debug_routes).  No HIP headers: the baseline planner
// (baseline_plan.hpp) names them, and its CPU test compiles without the library.
#pragma once
#include <cstdint>

namespace pixo_capi {

// Which of the library's forms served the calls since the record was last cleared: every decision point ORs its bit
// into one process-wide word (one relaxed fetch_or per decision, nothing on the device).  pixo_amd/jpeg.py mirrors the names.
namespace route {
enum : uint64_t {
    FUSED = 1ull << 0,             // the fused pixel -> scan kernel (jpeg_pixels_code.hip), one uninterrupted scan
    FUSED_SEGMENTED = 1ull << 1,   // ... its segments: the images of a batch or restart intervals of whole MCU rows
    FUSED_DIRECT = 1ull << 2,      // ... storing straight into host memory the GPU can write
    TWO_KERNEL = 1ull << 3,        // coefficient kernel + scan_code (a tuple in HBM coded by the entropy stage)
    DENSE_STREAM_RULE = 1ull << 4, // the context's last file was dense: the fused kernel would have served, the two-kernel form did
    SINGLE_PASS_TUPLE = 1ull << 5, // the single-pass tuple coders of jpeg_scan_fused.hip
    MULTI_PASS = 1ull << 6,        // the multi-pass entropy kernels of jpeg_entropy.hip (baseline or progressive)
    FALLBACK = 1ull << 7,          // a single-pass launch gave up waiting: the job ran again with the multi-pass kernels (PNG dither: band by band)
    HOST_ENTROPY = 1ull << 8,      // the host twin of the scan coders (debug switch host_entropy)
    PIECES = 1ull << 9,            // a scan coded in pieces while the file travels (device_entropy_pieces)
    HOST_BANDS = 1ull << 10,       // ... with host pixels uploaded in bands
    DIRECT_STORES = 1ull << 11,    // the stuffing kernel stores straight into pinned host memory (baseline)
    RESTUFF_GROW = 1ull << 12,     // the output buffer was short: grown, the stuffing pass repeated
    CALLER_RETRY = 1ull << 13,     // the caller's storage was too small (PIXO_ERR_BUFFER_TOO_SMALL)
    COEF_PACKED = 1ull << 14,      // packed DCT / quantiser forms (jpeg_kernels.hip packed_launch)
    COEF_SCALAR = 1ull << 15,      // scalar forms
    LOAD_ALIGNED = 1ull << 16,     // coefficient kernel: 12-byte loads of aligned rows
    LOAD_FUNNEL = 1ull << 17,      // ... aligned dwords and shifts
    LOAD_BYTES = 1ull << 18,       // ... byte gathers (images narrower than 4 pixels)
    PROG_SINGLE_PASS = 1ull << 19, // progressive scans by the single-pass kernels
    PROG_DIRECT_SMALL = 1ull << 20, // ... stored straight into host memory (small progressive files after a small one)
    SIDE_STATS = 1ull << 21,       // preset 2, small images: the statistics on a second stream beside the search
    TRELLIS_LANE = 1ull << 22,     // trellis search: one lane per block
    TRELLIS_GROUP = 1ull << 23,    // ... eight lanes per block
    BATCH_FUSED = 1ull << 24,      // a batch through the fused kernel, every image a segment
    BATCH_TWO_KERNEL = 1ull << 25, // a batch through coefficient kernel + entropy stage
    SUB_BATCHES = 1ull << 26,      // a batch in several sub-batches over two contexts (resize and decode batches: one after the other on one stream)
    BANDS_MULTI = 1ull << 27,      // one image in bands over several devices (pixo_hip_jpeg_encode_multi)
    PNG_REGS = 1ull << 28,         // PNG filter kernel: adaptive strategies with the row in the registers of 256 threads
    PNG_GENERAL = 1ull << 29,      // ... the general form (fixed filters, or rows too long for registers)
    PNG_BIGRAMS_REGS = 1ull << 30, // ... bigrams with the row in registers
    PNG_BIGRAMS = 1ull << 31,      // ... bigrams, general form
    SEGMENTED_TUPLE = 1ull << 32,  // the single-pass tuple coders over byte-aligned segments (batches, restart intervals)
    PROG_MULTI_PASS = 1ull << 33,  // progressive scans by the multi-pass kernels
    PIECES_REDO = 1ull << 34,      // a scan in pieces outgrew its guesses (0xFF bytes, dense content) and was coded again in one piece
    PNG_REGS512 = 1ull << 35,      // PNG filter kernel: adaptive strategies, rows of 16-32 KiB in the registers of 512 threads
    RESIZE_NEAREST = 1ull << 36,   // resize: the nearest form of the point kernel (resize.hip)
    RESIZE_BILINEAR = 1ull << 37,  // ... its bilinear form
    RESIZE_LANCZOS3 = 1ull << 38,  // ... the two Lanczos3 passes
    PNG_BATCH = 1ull << 39,        // PNG batch entries: one DEFLATE, scan, compaction and CRC launch over all images of a sub-batch
    PNG_BATCH_FILTER = 1ull << 40, // ... and one filter launch over all their rows in front of it
    RESIZE_BATCH = 1ull << 41,     // resize batch entries: one launch per pass over all images of a sub-batch (beside the algorithm's bit)
    PNG_DECODE_BATCH = 1ull << 42, // PNG decode batch entries: one unfilter launch per filter unit and one convert launch per kernel form a sub-batch
    PNG_INFLATE_DEVICE = 1ull << 43, // ... with PIXO_DECODE_DEVICE_INFLATE: the streams of a sub-batch inflated in one launch (png_inflate.hip)
    PNG_INFLATE_HOST_REDO = 1ull << 44, // ... a stream the device did not vouch for was inflated again by the host, whose bytes replaced it
    PNG_IMAGES = 1ull << 45,       // PNG encode of images of individual sizes: one DEFLATE, scan, compaction and CRC launch over all images of a sub-batch
    PNG_IMAGES_FILTER = 1ull << 46, // ... and at least one image's rows went through a ragged filter launch (one per class of images)
    RESIZE_IMAGES = 1ull << 47,    // resize images entries: one flat launch per pass and pixel size over all images of a sub-batch (beside the algorithm's bit)
    JPEG_IMAGES = RESIZE_IMAGES << 1, // (bit 48) JPEG encode of images of individual sizes: at least one sub-batch went through the ragged launches (beside TWO_KERNEL, SEGMENTED_TUPLE)
    JPEG_IMAGES_DIRECT = JPEG_IMAGES << 1, // (bit 49) ... and a sub-batch's scans travelled file by file straight into pinned destinations (large files: pool blocks or a pinned arena)
    JPEG_ENTROPY_DEVICE = JPEG_IMAGES_DIRECT << 1, // (bit 50) JPEG decode batch entries with PIXO_DECODE_DEVICE_ENTROPY: at least one scan of the call was decoded on the device (jpeg_entropy_dec.hip)
    JPEG_ENTROPY_HOST_REDO = JPEG_ENTROPY_DEVICE << 1, // (bit 51) ... at least one file the device did not vouch for was decoded by the host, whose coefficients or whose refusal stood
};
}

} // namespace pixo_capi
