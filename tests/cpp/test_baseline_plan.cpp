// plan_baseline_file (pixo_amd/csrc/baseline_plan.hpp) table-tested without the library: every decision the whole-file
// executor makes before it launches anything.  Built and run by tests/test_baseline_plan.py.
#include <cstdio>
#include <functional>

#include "../../pixo_amd/csrc/baseline_plan.hpp"

using namespace pixo_capi;
using Form = BaselinePlan::Form;
using Direct = BaselinePlan::Direct;
using Upload = BaselinePlan::Upload;

namespace {

// 4:2:0 images: 6 blocks per 16x16 MCU.  Groups of 192 blocks: 4096 groups = 2 x piece_groups (large), 1024 = piece_medium.
constexpr uint64_t kLarge = 4096 * 192, kJustNotLarge = 4095 * 192, kMedium = 1024 * 192, kJustNotMedium = 1023 * 192;
constexpr uint64_t kMiB = uint64_t{1} << 20;

// One RGB image from device pixels that the fused kernel can code, into the context's pinned buffer, no history.
PlanFacts device_pixels(uint64_t blocks)
{
    PlanFacts f;
    f.blocks = blocks;
    f.fused = true;
    f.pixels = true;
    f.pixel_bytes = blocks * 32; // (4:2:0: 6 blocks per 256 pixels of 3 bytes)
    f.pixels_code_usable = true;
    return f;
}
PlanFacts tuple(uint64_t blocks)
{
    PlanFacts f = device_pixels(blocks);
    f.pixels = f.pixels_code_usable = false;
    return f;
}
PlanFacts with(PlanFacts f, const std::function<void(PlanFacts &)> &change)
{
    change(f);
    return f;
}
void history(PlanFacts &f, uint64_t bytes, uint64_t blocks)
{
    f.last_scan_bytes = bytes;
    f.last_scan_blocks = blocks;
}
void caller(PlanFacts &f, size_t cap, bool gpu_writable)
{
    f.dest = DestKind::Caller;
    f.dest_cap = cap;
    f.dest_gpu_writable = gpu_writable;
}
void host(PlanFacts &f, uint64_t pixel_bytes)
{
    f.host_pixels = true;
    f.pixel_bytes = pixel_bytes;
}

struct Case {
    const char *name;
    PlanFacts f;
    Form form;
    Direct direct;
    Upload upload;
    bool coeffs_first;
    uint64_t notes;
};

const char *form_name(Form f)
{
    return f == Form::Pieces ? "pieces" : f == Form::Pixels ? "pixels" : f == Form::SinglePass ? "single-pass" : "multi-pass";
}

} // namespace

int main()
{
    const size_t room = pieces_file_bound(kLarge); // caller storage that holds any file the pieces are sized for
    const Case cases[] = {
        // ---- small, medium and large scans from device pixels / from the tuple -----------------------------------------------
        {"small device pixels -> pinned", device_pixels(4096), Form::Pixels, Direct::PinnedBuffer, Upload::None, false, 0},
        {"large device pixels -> pinned: one kernel storing direct", device_pixels(kLarge), Form::Pixels, Direct::PinnedBuffer, Upload::None, false, 0},
        {"just below large, no history -> pinned", device_pixels(kJustNotLarge), Form::Pixels, Direct::PinnedBuffer, Upload::None, false, 0},
        {"large tuple -> pinned: pieces", tuple(kLarge), Form::Pieces, Direct::None, Upload::None, false, 0},
        {"just below large tuple, no history: one piece", tuple(kJustNotLarge), Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"large device pixels -> roomy pageable caller: pieces", with(device_pixels(kLarge), [&](PlanFacts &f) { caller(f, room, false); }),
         Form::Pieces, Direct::None, Upload::None, false, 0},
        {"large device pixels -> pageable caller one byte short of the bound", with(device_pixels(kLarge), [&](PlanFacts &f) { caller(f, room - 1, false); }),
         Form::Pixels, Direct::None, Upload::None, false, 0},
        {"large device pixels -> GPU-writable caller", with(device_pixels(kLarge), [&](PlanFacts &f) { caller(f, room, true); }),
         Form::Pixels, Direct::CallerStorage, Upload::None, false, 0},
        {"large device pixels -> small GPU-writable caller", with(device_pixels(kLarge), [&](PlanFacts &f) { caller(f, 4096, true); }),
         Form::Pixels, Direct::CallerStorage, Upload::None, false, 0},
        {"large device pixels, size query", with(device_pixels(kLarge), [&](PlanFacts &f) { caller(f, 0, false); }),
         Form::Pixels, Direct::None, Upload::None, false, 0},
        {"large tuple, size query", with(tuple(kLarge), [&](PlanFacts &f) { caller(f, 0, false); }),
         Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"large tuple -> roomy pageable caller: pieces", with(tuple(kLarge), [&](PlanFacts &f) { caller(f, room, false); }),
         Form::Pieces, Direct::None, Upload::None, false, 0},
        {"small tuple -> GPU-writable caller", with(tuple(4096), [&](PlanFacts &f) { caller(f, 1 << 20, true); }),
         Form::SinglePass, Direct::CallerStorage, Upload::None, false, 0},
        {"small tuple -> pageable caller", with(tuple(4096), [&](PlanFacts &f) { caller(f, 1 << 20, false); }),
         Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"large tuple -> own block: never pieces", with(tuple(kLarge), [](PlanFacts &f) { f.dest = DestKind::OwnBlock; }),
         Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"large device pixels -> own block", with(device_pixels(kLarge), [](PlanFacts &f) { f.dest = DestKind::OwnBlock; }),
         Form::Pixels, Direct::PinnedBuffer, Upload::None, false, 0},
        {"small tuple -> own block: direct into the pinned buffer", with(tuple(4096), [](PlanFacts &f) { f.dest = DestKind::OwnBlock; }),
         Form::SinglePass, Direct::PinnedBuffer, Upload::None, false, 0},
        {"large device pixels, optimised tables -> pageable caller: tuple first, pieces",
         with(device_pixels(kLarge), [&](PlanFacts &f) { caller(f, room, false); f.optimize_huffman = true; }),
         Form::Pieces, Direct::None, Upload::None, true, 0},
        // ---- the medium rule: 12 bytes per block of the last scan ------------------------------------------------------------
        {"medium tuple after 12 B/block: pieces", with(tuple(kMedium), [](PlanFacts &f) { history(f, 12 * 1000, 1000); }),
         Form::Pieces, Direct::None, Upload::None, false, 0},
        {"medium tuple after just under 12 B/block", with(tuple(kMedium), [](PlanFacts &f) { history(f, 12 * 1000 - 1, 1000); }),
         Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"medium tuple, no history", tuple(kMedium), Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"just below medium tuple after 12 B/block", with(tuple(kJustNotMedium), [](PlanFacts &f) { history(f, 12 * 1000, 1000); }),
         Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"medium device pixels after 12 B/block: the fused kernel", with(device_pixels(kMedium), [](PlanFacts &f) { history(f, 12 * 1000, 1000); }),
         Form::Pixels, Direct::PinnedBuffer, Upload::None, false, 0},
        {"medium tuple, piece_medium forced", with(tuple(kMedium), [](PlanFacts &f) { f.piece_medium_forced = true; }),
         Form::Pieces, Direct::None, Upload::None, false, 0},
        {"piece_medium=2 on a small tuple", with(tuple(4096), [](PlanFacts &f) { f.piece_medium = 2; f.piece_medium_forced = true; }),
         Form::Pieces, Direct::None, Upload::None, false, 0},
        {"piece_groups=1: 3 groups (tuple)", with(tuple(385), [](PlanFacts &f) { f.piece_groups = 1; }),
         Form::Pieces, Direct::None, Upload::None, false, 0},
        {"piece_groups=1: 2 groups are large (tuple)", with(tuple(384), [](PlanFacts &f) { f.piece_groups = 1; }),
         Form::Pieces, Direct::None, Upload::None, false, 0},
        {"piece_groups=1: 1 group (tuple)", with(tuple(192), [](PlanFacts &f) { f.piece_groups = 1; }),
         Form::SinglePass, Direct::PinnedBuffer, Upload::None, false, 0},
        {"piece_groups=1, device pixels -> pinned", with(device_pixels(385), [](PlanFacts &f) { f.piece_groups = 1; }),
         Form::Pixels, Direct::PinnedBuffer, Upload::None, false, 0},
        // ---- the dense-stream rule: more than 30 bytes per block of the last scan -----------------------------------------------
        {"large device pixels after 31 B/block: two kernels, pieces", with(device_pixels(kLarge), [](PlanFacts &f) { history(f, 31 * 1000, 1000); }),
         Form::Pieces, Direct::None, Upload::None, false, route::DENSE_STREAM_RULE},
        {"large device pixels after 30 B/block: the fused kernel", with(device_pixels(kLarge), [](PlanFacts &f) { history(f, 30 * 1000, 1000); }),
         Form::Pixels, Direct::PinnedBuffer, Upload::None, false, 0},
        {"small device pixels after 31 B/block", with(device_pixels(4096), [](PlanFacts &f) { history(f, 31 * 1000, 1000); }),
         Form::SinglePass, Direct::PinnedBuffer, Upload::None, true, route::DENSE_STREAM_RULE},
        {"dense history, pixels the fused kernel cannot code", with(device_pixels(4096), [](PlanFacts &f) { history(f, 31 * 1000, 1000); f.pixels_code_usable = false; }),
         Form::SinglePass, Direct::PinnedBuffer, Upload::None, true, 0},
        {"dense history under fused_batch", with(device_pixels(4096), [](PlanFacts &f) { history(f, 31 * 1000, 1000); f.fused_batch = true; }),
         Form::Pixels, Direct::PinnedBuffer, Upload::None, false, 0},
        {"dense history, tuple: no note", with(tuple(kLarge), [](PlanFacts &f) { history(f, 31 * 1000, 1000); }),
         Form::Pieces, Direct::None, Upload::None, false, 0},
        // ---- host pixels: bands from 96 MiB on ---------------------------------------------------------------------------------
        {"96 MiB host pixels -> own block: pieces, bands", with(device_pixels(kLarge), [](PlanFacts &f) { host(f, 96 * kMiB); f.dest = DestKind::OwnBlock; }),
         Form::Pieces, Direct::None, Upload::Bands, false, 0},
        {"96 MiB - 1 host pixels -> own block", with(device_pixels(kLarge), [](PlanFacts &f) { host(f, 96 * kMiB - 1); f.dest = DestKind::OwnBlock; }),
         Form::Pixels, Direct::PinnedBuffer, Upload::OneCopy, false, 0},
        {"96 MiB host pixels -> pageable caller one byte short", with(device_pixels(kLarge), [&](PlanFacts &f) { host(f, 96 * kMiB); caller(f, room - 1, false); }),
         Form::Pixels, Direct::None, Upload::OneCopy, false, 0},
        {"96 MiB host pixels, optimised tables: one copy, tuple first", with(device_pixels(kLarge), [](PlanFacts &f) { host(f, 96 * kMiB); f.optimize_huffman = true; }),
         Form::Pieces, Direct::None, Upload::OneCopy, true, 0},
        {"96 MiB host pixels, no_bands_upload", with(device_pixels(kLarge), [](PlanFacts &f) { host(f, 96 * kMiB); f.no_bands_upload = true; }),
         Form::Pixels, Direct::PinnedBuffer, Upload::OneCopy, false, 0},
        {"bands_upload_min_mb=1, 1 MiB of host pixels", with(device_pixels(24576), [](PlanFacts &f) { host(f, kMiB); f.bands_upload_min_mb = 1; f.dest = DestKind::OwnBlock; }),
         Form::Pieces, Direct::None, Upload::Bands, false, 0},
        {"large host pixels below the bands -> roomy pageable caller: one copy, pieces",
         with(device_pixels(kLarge), [&](PlanFacts &f) { host(f, 48 * kMiB); caller(f, room, false); }),
         Form::Pieces, Direct::None, Upload::OneCopy, false, 0},
        {"small host pixels -> pageable caller", with(device_pixels(4096), [](PlanFacts &f) { host(f, 3 * kMiB / 16); caller(f, 1 << 20, false); }),
         Form::Pixels, Direct::None, Upload::OneCopy, false, 0},
        // ---- direct stores: 32,768 blocks / 768 KB predicted --------------------------------------------------------------------
        {"32768-block tuple", tuple(32768), Form::SinglePass, Direct::PinnedBuffer, Upload::None, false, 0},
        {"32769-block tuple, no history", tuple(32769), Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"100000 blocks after 7.5 B/block (750 KB predicted)", with(tuple(100000), [](PlanFacts &f) { history(f, 75, 10); }),
         Form::SinglePass, Direct::PinnedBuffer, Upload::None, false, 0},
        {"100000 blocks after 8 B/block (800 KB predicted)", with(tuple(100000), [](PlanFacts &f) { history(f, 80, 10); }),
         Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"no_direct_small, small tuple", with(tuple(4096), [](PlanFacts &f) { f.no_direct_small = true; }),
         Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"no_direct_small, small device pixels", with(device_pixels(4096), [](PlanFacts &f) { f.no_direct_small = true; }),
         Form::Pixels, Direct::None, Upload::None, false, 0},
        {"no_direct_small, large device pixels -> pinned: pieces", with(device_pixels(kLarge), [](PlanFacts &f) { f.no_direct_small = true; }),
         Form::Pieces, Direct::None, Upload::None, false, 0},
        {"direct_stores, large tuple", with(tuple(kLarge), [](PlanFacts &f) { f.direct_stores = true; }),
         Form::SinglePass, Direct::PinnedBuffer, Upload::None, false, 0},
        {"one_piece, large tuple", with(tuple(kLarge), [](PlanFacts &f) { f.one_piece = true; }),
         Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"restart intervals as segments", with(tuple(4096), [](PlanFacts &f) { f.segmented = true; }),
         Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"large tuple, segmented: no pieces", with(tuple(kLarge), [](PlanFacts &f) { f.segmented = true; }),
         Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"short restart intervals: multi-pass", with(tuple(4096), [](PlanFacts &f) { f.fused = false; }),
         Form::MultiPass, Direct::None, Upload::None, false, 0},
        {"multi-pass retry from device pixels", with(device_pixels(kLarge), [](PlanFacts &f) { f.fused = false; f.pixels_code_usable = false; }),
         Form::MultiPass, Direct::None, Upload::None, true, 0},
        // ---- batches (scans left in HBM) -------------------------------------------------------------------------------------
        {"batch through the fused kernel", with(device_pixels(64 * 4096), [](PlanFacts &f) { f.batch = 64; f.segmented = true; f.dest = DestKind::InHbm; }),
         Form::Pixels, Direct::None, Upload::None, false, route::BATCH_FUSED},
        {"batch through the two-kernel form", with(device_pixels(64 * 4096), [](PlanFacts &f) { f.batch = 64; f.segmented = true; f.dest = DestKind::InHbm; f.pixels_code_usable = false; }),
         Form::SinglePass, Direct::None, Upload::None, true, route::BATCH_TWO_KERNEL},
        {"batch after a dense file: no dense rule", with(device_pixels(64 * 4096), [](PlanFacts &f) { f.batch = 64; f.segmented = true; f.dest = DestKind::InHbm; history(f, 31 * 1000, 1000); }),
         Form::Pixels, Direct::None, Upload::None, false, route::BATCH_FUSED},
        {"large batch: never pieces", with(device_pixels(kLarge), [](PlanFacts &f) { f.batch = 2; f.segmented = true; f.dest = DestKind::InHbm; f.pixels_code_usable = false; }),
         Form::SinglePass, Direct::None, Upload::None, true, route::BATCH_TWO_KERNEL},
        {"batch, multi-pass", with(device_pixels(64 * 4096), [](PlanFacts &f) { f.batch = 64; f.fused = false; f.dest = DestKind::InHbm; f.pixels_code_usable = false; }),
         Form::MultiPass, Direct::None, Upload::None, true, route::BATCH_TWO_KERNEL},
        // ---- a pieces attempt that started over: planned again from the tuple, in one piece ---------------------------------
        {"after pieces of host bands", tuple_computed_no_pieces(with(device_pixels(kLarge), [](PlanFacts &f) { host(f, 96 * kMiB); f.dest = DestKind::OwnBlock; })),
         Form::SinglePass, Direct::None, Upload::None, false, 0},
        {"after pieces, a small file predicted", tuple_computed_no_pieces(with(tuple(kLarge), [](PlanFacts &f) { history(f, 1, 1000); })),
         Form::SinglePass, Direct::PinnedBuffer, Upload::None, false, 0},
        {"after pieces into a roomy GPU-writable caller, dense history",
         tuple_computed_no_pieces(with(device_pixels(kLarge), [&](PlanFacts &f) { caller(f, room, true); history(f, 31 * 1000, 1000); })),
         Form::SinglePass, Direct::None, Upload::None, false, 0},
    };
    int failures = 0, n = 0;
    for (const Case &k : cases) {
        ++n;
        const BaselinePlan p = plan_baseline_file(k.f);
        if (p.form != k.form || p.direct != k.direct || p.upload != k.upload || p.coeffs_first != k.coeffs_first || p.notes != k.notes) {
            ++failures;
            std::printf("FAIL %s: form %s (want %s), direct %d (%d), upload %d (%d), coeffs_first %d (%d), notes %#llx (%#llx)\n", k.name,
                        form_name(p.form), form_name(k.form), static_cast<int>(p.direct), static_cast<int>(k.direct), static_cast<int>(p.upload),
                        static_cast<int>(k.upload), p.coeffs_first, k.coeffs_first, static_cast<unsigned long long>(p.notes),
                        static_cast<unsigned long long>(k.notes));
        }
    }
    // the bound the pieces' caller storage must reach: 64 bytes per block + room for headers and slack
    if (pieces_file_bound(1000) != 1024 + 64000 + 8192) { ++failures; std::printf("FAIL pieces_file_bound\n"); }
    if (failures) return 1;
    std::printf("%d cases, all checks passed\n", n);
    return 0;
}
