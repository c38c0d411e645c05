// baseline_plan.hpp — which route a whole baseline file takes (baseline_file.cpp runs it).  Plain values in, a plan out: no HIP
// headers, no context, nothing launched — tests/test_baseline_plan.py compiles it with g++ alone and table-tests every rule.
#pragma once
#include <cstddef>
#include <cstdint>

#include "routes.hpp"

namespace pixo_capi {

// Where a finished file goes (FileDest, capi_internal.hpp).
enum class DestKind : uint8_t {
    Caller,   // the caller's storage (cap == 0: a size query)
    OwnBlock, // a block the caller will own (pixo_hip_free)
    Pinned,   // the context's pinned file buffer
    InHbm,    // nowhere: the scans of a batch stay in c.e_out, the caller delivers them
};

// What the route depends on, known before anything is launched: the scan job after scan_begin, the source, the destination,
// the context's last scan and the debug switches that bear on it.
struct PlanFacts {
    uint64_t blocks = 0;             // j.n (all images of a batch)
    bool fused = false;              // j.fused: the single-pass tuple coders serve this job
    bool segmented = false;          // j.segmented: ... as byte-aligned segments (batch images, restart intervals)
    uint32_t batch = 1;
    bool pixels = false;             // pixels given, the tuple not computed yet (PixelSource)
    bool host_pixels = false;        // ... still in host memory
    uint64_t pixel_bytes = 0;        // of one image
    bool pixels_code_usable = false; // the fused pixel -> scan kernel can code this job (scan_job.cpp pixels_code_usable)
    bool optimize_huffman = false;
    DestKind dest = DestKind::Pinned;
    size_t dest_cap = 0;             // Caller: bytes available
    bool dest_gpu_writable = false;  // Caller: pinned / registered storage the GPU can store into
    uint64_t last_scan_bytes = 0, last_scan_blocks = 0; // the context's last whole scan (0 blocks: none yet)
    // debug switches (capi_internal.hpp DebugSwitches)
    bool one_piece = false, direct_stores = false, no_direct_small = false, fused_batch = false, no_bands_upload = false;
    uint32_t bands_upload_min_mb = 96;
    uint64_t piece_groups = 2048, piece_medium = 1024;
    bool piece_medium_forced = false;
};

struct BaselinePlan {
    enum class Form : uint8_t {
        Pieces,     // a scan coded in pieces while the file travels (device_entropy_pieces)
        Pixels,     // the fused pixel -> scan kernel, one launch (scan_from_pixels); the tuple is never written
        SinglePass, // the single-pass tuple coders: code + stuff back to back (scan_stuff_fused)
        MultiPass,  // the multi-pass tuple coders (scan_lengths + scan_pack)
    };
    enum class Direct : uint8_t { None, PinnedBuffer, CallerStorage }; // where the stuffing kernel stores straight into host memory
    enum class Upload : uint8_t { None, OneCopy, Bands };              // how host pixels reach the device
    Form form = Form::MultiPass;
    Direct direct = Direct::None; // (CallerStorage: only if it holds more than the headers + EOI, known once the tables are)
    Upload upload = Upload::None;
    bool coeffs_first = false;    // the coefficient kernel over the whole image (batch) before the entropy stage
    uint64_t notes = 0;           // route bits of the decision (route::DIRECT_STORES is noted where the stores go direct)
};

// Bytes that hold any file whose scan the stuffing grids of the pieces are sized for (a block has at most 64 bytes there).
inline uint64_t pieces_file_bound(uint64_t blocks) { return 1024 + blocks * 64 + 8192; }

inline BaselinePlan plan_baseline_file(const PlanFacts &f)
{
    using Form = BaselinePlan::Form;
    BaselinePlan p;
    const bool caller = f.dest == DestKind::Caller;
    const bool one_file = f.batch == 1 && f.dest != DestKind::InHbm; // (a file finished in host memory: pieces and direct stores may serve)
    // A large scan is coded in pieces so that the file's way to the host overlaps the coding (pieces.cpp).  A piece is at least
    // piece_groups (2048) groups of 192 blocks, and a scan of fewer than two such pieces is not cut into equal pieces.  2048
    // groups = the scan of a 4096x4096 4:2:0 image: the kernels of a smaller piece are mostly start-up — a sixth of that scan
    // takes 28 us where the whole takes 52 — and a 4096x4096 image in 2 or 6 equal pieces is no faster than in one (0.30-0.33
    // against 0.31 ms); a 16384x16384 scan in 16 such pieces hides its 1 ms of coding behind 3.4 ms of PCIe.
    const uint64_t groups = (f.blocks + 191) / 192;
    const bool large = groups >= 2 * f.piece_groups;
    // Medium scans (piece_medium (1024) <= groups < 2 piece_groups) in a few pieces that grow only pay when the file is large (a
    // 0.3 MB file of a smooth 4096x4096 image: 0.12 ms in one piece, more in two): the context's last scan decides — 12 bytes per
    // block or more (a stream of similar images; the first one is coded in one piece).
    const bool medium = !large && groups >= f.piece_medium &&
                        ((f.last_scan_blocks && f.last_scan_bytes >= 12 * f.last_scan_blocks) || f.piece_medium_forced);
    // Pixels still in host memory (pixo_hip_jpeg_encode / _encode_into): their way over PCIe is most of the call.  From 96 MB of
    // pixels on (8192x4096) the image is uploaded in bands, each band transformed and coded while the next one travels, coded
    // pieces on their way back meanwhile (device_entropy_pieces): 16384x16384 17.7 -> 15.1 ms, which is the upload alone at
    // 53 GB/s.  Below that the two extra threads' hand-offs cost what the overlap gains (4096x4096: 1.18 ms either way, of which
    // 0.95 are the upload; profiles/r03_host_pipeline.txt).  Whatever the route, the pixels are uploaded once.
    const bool host_bands = f.host_pixels && f.pixel_bytes >= (uint64_t{f.bands_upload_min_mb} << 20) && !f.no_bands_upload;
    // Round 5: pixels that have not been transformed yet go through the fused pixel -> bit stream kernel (jpeg_pixels_code.hip)
    // where that kernel serves the job — one piece: the whole scan is coded ~50 us after the call began, which is where the first
    // of a medium scan's pieces used to be.  Large scans and host pixels in bands keep the pieces (their PCIe time is what the
    // pieces hide); their bands run coefficient kernel + scan_code as before.
    // (A stream of files of more than 30 bytes per block — 4:2:0 above 5.6 bit/px: photographs at q = 100, noise at q >= 90 — would
    // run the fused kernel's two-pass form for groups of several rounds, 25-50 % behind the two-kernel form: the context's last
    // file decides, as it does for the pieces.  profiles/r06_long_groups_chain.txt)
    const bool dense_stream = f.batch == 1 && f.last_scan_blocks && f.last_scan_bytes > 30 * f.last_scan_blocks && !f.fused_batch;
    const bool from_pixels = f.pixels && f.pixels_code_usable && !dense_stream;
    if (f.pixels && f.pixels_code_usable && dense_stream) p.notes |= route::DENSE_STREAM_RULE;
    if (f.batch > 1) p.notes |= from_pixels ? route::BATCH_FUSED : route::BATCH_TWO_KERNEL;
    // Second session of round 6: a LARGE scan from device pixels takes the fused kernel too when its stores can go straight to
    // where the file is wanted (the library's pinned buffer, or storage of the caller's the GPU can write) — one kernel whose
    // groups finish one after the other IS a pipeline of coding and PCIe: 4096x4096 4:4:4 photo 181 -> 121 us, gradient
    // 144 -> 88, noise 534 -> 498; 8192x8192 4:2:0 332 -> 261 / 264 -> 152 / 928 -> 916 (tools/large_scan_paths.py,
    // profiles/r06_large_scans_one_kernel.txt).  Plain malloc'd destinations keep the pieces (their copy engine overlaps the
    // coding), host pixels in bands as well.
    const bool fused_direct = from_pixels && one_file && large && !host_bands && !f.no_direct_small && (!caller || f.dest_gpu_writable);
    // Pieces go into the context's pinned buffer, or into the caller's storage if that can hold any file the stuffing grids are
    // sized for (a smaller one might not fit the file, and then nothing may have been written to it: one piece, size first).
    // Not for a caller that wants a block of its own: the block would have to be allocated before the size is known — 64 bytes
    // per block, cut to size afterwards — and a block of a new size is new pages every call, which the device-to-host copy has
    // to fault in and pin: 20 ms instead of 0.7 for the 4096x4096 noise image.  One piece, the exact size, recycled by malloc.
    const bool pieces = f.fused && !f.segmented && one_file && !f.one_piece && !f.direct_stores &&
                        ((large && !fused_direct) || (medium && !from_pixels) || host_bands) &&
                        (!caller || f.dest_cap >= pieces_file_bound(f.blocks)) && (host_bands || f.dest != DestKind::OwnBlock);
    if (pieces) {
        p.form = Form::Pieces;
        p.coeffs_first = f.pixels && f.optimize_huffman; // (the statistics need the whole tuple)
        if (f.host_pixels) p.upload = host_bands && !p.coeffs_first ? BaselinePlan::Upload::Bands : BaselinePlan::Upload::OneCopy;
        return p;
    }
    p.form = from_pixels ? Form::Pixels : (f.fused ? Form::SinglePass : Form::MultiPass);
    p.coeffs_first = f.pixels && !from_pixels;
    if (f.host_pixels) p.upload = BaselinePlan::Upload::OneCopy;
    if (p.form == Form::MultiPass || !one_file || f.segmented) return p;
    // One image into host memory the GPU can write — the context's pinned file buffer, or storage of the caller's that is pinned
    // / registered: the stuffing kernel stores straight into it, behind the place of the headers.  Small files take that way by
    // default: the stuffing kernel's stores ARE the transfer, and the call has one wait instead of wait + copy + wait — 64x64
    // 62 -> 42 us, 512x512 noise 65 -> 54 us (device pixels -> pinned), any smooth 1080p image 59 -> 48 us; a 1.4 MB file (1080p
    // noise) is where the copy engine wins again (profiles/r04_small_latency.txt).  "Small" = at most 32,768 blocks (1024x1365
    // px at 4:2:0), or a file predicted below 768 KB from the bytes per block of this context's last scan.  Large files: the
    // debug switch `direct_stores` (slower, profiles/r02_direct_host_stores.txt).
    constexpr uint64_t kDirectBlocks = 32768, kDirectBytes = 768u << 10;
    const bool small_file = !f.no_direct_small &&
                            (f.blocks <= kDirectBlocks ||
                             (f.last_scan_blocks && static_cast<double>(f.blocks) * static_cast<double>(f.last_scan_bytes) /
                                                            static_cast<double>(f.last_scan_blocks) <= kDirectBytes));
    // The one-kernel form (round 5) stores directly at EVERY size: its groups finish one after the other, so the stores of the
    // early ones cross PCIe while the late ones are still coding — 4096x4096 photo-like content 0.129 -> 0.112 ms, noise (11 MB,
    // PCIe-bound either way) 0.291 -> 0.283 ms against kernel + copy engine (profiles/r05_whole_file.txt).
    if (f.direct_stores || small_file || (from_pixels && !f.no_direct_small)) {
        if (!caller) p.direct = BaselinePlan::Direct::PinnedBuffer;
        else if (f.dest_gpu_writable) p.direct = BaselinePlan::Direct::CallerStorage;
    }
    return p;
}

// A pieces attempt that started over (its stream outgrew the guesses) has computed the tuple and uploaded any host pixels: the
// file is planned again from the tuple, in one piece.
inline PlanFacts tuple_computed_no_pieces(PlanFacts f)
{
    f.pixels = f.host_pixels = false;
    f.one_piece = true;
    return f;
}

} // namespace pixo_capi
