// jpeg_decode_api.cpp — the extern "C" JPEG decode entry points (pixo::decode::decode_jpeg, reference src/decode/jpeg.rs:738):
// the marker walk and the entropy decode on the host (jpeg_decode_host.cpp), dequantisation, IDCT, upsampling, colour conversion
// and the crop on the device (jpeg_decode.hip).  N files -> N images back to back in device memory, described by the records the
// PNG decode batch fills in (pixo_png_image); the single entries are the batch of one, their refusals without " (image 0)".
//
// Two phases of checks, both before anything is enqueued.  Phase 1, per file in index order: the walk from SOI to SOS.  In the
// reference's order and words: "not a JPEG file"; per marker "unexpected end of file", "truncated marker", "invalid marker
// length", then the segment's own checks (SOF0: length, precision, component count, truncation, sampling factors of zero, table
// id; SOF2: progressive; DHT, DQT, DRI: table ids and lengths; SOS: empty, component count, truncation, table ids); "no image
// data found" at EOI.  Ours, at SOS behind the reference's: no frame yet; a sampling other than 4:4:4 / 4:2:2 / 4:2:0
// (Unsupported); a scan whose components are not the frame's in order (Unsupported); an Adobe transform other than 1 on three
// components (Unsupported); component ids R, G, B (Unsupported); a quantisation or Huffman table the scan uses and no segment
// defined; a scan shorter than two bits per block.  Ours at DHT: code lengths that describe no prefix code.  Phase 2, the
// entropy decodes on up to 8 host threads (PIXO_DECODE_ONE_THREAD: on the caller): a scan that breaks off, a code no table
// holds, a coefficient index past 63, a missing or out-of-sequence RSTn.  The failing file with the lowest index answers.
// A width or height of zero is no special case: such an image has no MCUs, no tiles and no bytes.
// With PIXO_DECODE_DEVICE_ENTROPY (the batch entries; opt-in) phase 2 changes: the scans are decoded on the device
// (jpeg_entropy_dec.hip), which vouches for a file or does not; what it does not vouch for, and what it is never sent, the host
// decodes, and the host's coefficients or refusal stand — decode_batch_device_entropy below.  Those refusals come behind the
// sub-batch's entropy launches.
// The steps every batch driver takes, and their order: DESIGN.md §4.0; the shared ones: batch_steps.hpp.
#include "batch_steps.hpp"
#include "jpeg_decode.hpp"
#include "jpeg_decode_host.hpp"
#include "jpeg_entropy_dec.hpp"
#include "jpeg_entropy_dec_host.hpp"

#include <algorithm>
#include <atomic>

using namespace pixo_capi;
namespace jd = pixo_jdec;
namespace jh = pixo_jdec_host;
namespace je = pixo_jent;

namespace {

constexpr uint64_t kDecodeBatchBytes = uint64_t{512} << 20; // coefficients one sub-batch holds at most (debug switch decode_batch_bytes)
constexpr uint32_t kDecodeBatchThreads = 8;                 // host threads that decode a batch's scans, the caller among them, at most

int status_of(jh::Kind k, const std::string &msg, const std::string &where)
{
    if (k == jh::OK) return PIXO_OK;
    return k == jh::UNSUPPORTED ? fail(PIXO_ERR_UNSUPPORTED_DECODE, "Unsupported: " + msg + where) : fail(PIXO_ERR_INVALID_DECODE, "Decode error: " + msg + where);
}

struct DecodeBatch {
    std::vector<jh::File> files;
    std::vector<pixo_png_image> images;
    std::vector<uint64_t> coef_at; // where each image's coefficients start in the call's staging (multiples of 8192)
    uint64_t total = 0, staging = 0;
    uint32_t threads = 1;
    bool single = false; // a single entry: refusals carry no " (image 0)"
    double entropy_ms = 0;
    std::string where(uint32_t i) const { return single ? std::string() : pixo_capi::where(i); }
};

// Phase 1 behind `files` and `batch`: per file its `data`, then the walk; the block's layout.  No HIP, no entropy decode.
int batch_walk(const pixo_png_file *files, uint32_t batch, DecodeBatch &b)
{
    b.files.resize(batch);
    b.images.resize(batch);
    b.coef_at.resize(batch);
    for (uint32_t i = 0; i < batch; ++i) {
        if (!files[i].data) return fail(PIXO_ERR_COMPRESSION, "Compression error: null argument 'data'" + b.where(i));
        std::string msg;
        const jh::Kind k = jh::walk(files[i].data, files[i].len, b.files[i], &msg);
        if (const int rc = status_of(k, msg, b.where(i))) return rc;
    }
    uint64_t at = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        const jh::File &f = b.files[i];
        b.coef_at[i] = b.staging;
        b.staging += f.coef_bytes();
        b.images[i] = lay_out(at, f.width, f.height, f.color_type(), &b.total);
    }
    return PIXO_OK;
}

// Phase 2: every scan decoded to stage + coef_at on up to kDecodeBatchThreads threads, which hand back (kind, message) — fail()
// is the calling thread's; the failing file with the lowest index decides, whoever decoded it.
int batch_entropy(DecodeBatch &b, uint8_t *stage, uint32_t flags)
{
    const uint32_t batch = static_cast<uint32_t>(b.files.size());
    b.threads = (flags & PIXO_DECODE_ONE_THREAD) ? 1u : std::min(batch, kDecodeBatchThreads);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<jh::Kind> kind(batch, jh::OK);
    std::vector<std::string> msg(batch);
    std::atomic<uint32_t> next{0};
    run_on_threads(b.threads, [&](unsigned) {
        for (uint32_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < batch;)
            kind[i] = jh::entropy_decode(b.files[i], reinterpret_cast<int16_t *>(stage + b.coef_at[i]), &msg[i]);
    });
    b.entropy_ms = ms_since(t0);
    for (uint32_t i = 0; i < batch; ++i)
        if (const int rc = status_of(kind[i], msg[i], b.where(i))) return rc;
    return PIXO_OK;
}

// What the driver decided, before anything touches a device (also: pixo_hip_debug_jpeg_decode_batch_plan)
struct DecodePlan {
    SubBatches sub_first;
    struct Launch { uint32_t sub, cls, form, first_record, count, tiles; };
    std::vector<Launch> launches;      // in stream order
    std::vector<jd::Record> records;   // launch after launch
    std::vector<uint32_t> record_image; // the image each record was made from
    uint64_t coef_bytes = 0;           // the largest sub-batch's
    // PIXO_DECODE_DEVICE_ENTROPY: the files whose scans go to the device, and the largest sub-batch's needs
    std::vector<uint8_t> on_device;
    uint64_t scan_bytes = 0, subs = 0, groups = 0, device_files = 0;
};
// What a file's record and scan take of a sub-batch's upload (the scan padded to 16 bytes and 16 more)
inline uint64_t scan_upload_bytes(const jh::File &f) { return sizeof(je::FileRecord) + round16(f.ecs_len) + 16; }
// d_pixels: the address the offsets count from (the plan entry: 0, any 16-byte aligned block)
int decode_plan(const DecodeBatch &b, uintptr_t d_pixels, uint32_t flags, DecodePlan &p)
{
    const uint32_t batch = static_cast<uint32_t>(b.files.size());
    const uint64_t limit = debug().decode_batch_bytes ? debug().decode_batch_bytes : kDecodeBatchBytes;
    const bool device_entropy = (flags & PIXO_DECODE_DEVICE_ENTROPY) != 0;
    p.on_device.assign(batch, 0);
    uint64_t held = 0, scans = 0, subs = 0, groups = 0, device_files = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        const jh::File &f = b.files[i];
        p.on_device[i] = device_entropy && je::device_takes(f);
        const uint64_t up = p.on_device[i] ? scan_upload_bytes(f) : 0;
        const uint64_t need = f.coef_bytes() + up; // (under the flag the scans' bytes count too)
        if (p.sub_first.starts_at(i, held + need > limit)) held = scans = subs = groups = device_files = 0;
        held += need;
        scans += up;
        p.coef_bytes = std::max(p.coef_bytes, held - scans);
        if (p.on_device[i]) {
            const uint32_t n = je::subs_of(static_cast<uint32_t>(f.ecs_len));
            subs += n; groups += je::groups_of(n); ++device_files;
            p.scan_bytes = std::max(p.scan_bytes, scans); p.subs = std::max(p.subs, subs); p.groups = std::max(p.groups, groups);
            p.device_files = std::max(p.device_files, device_files);
        }
    }
    p.sub_first.close(batch);
    for (uint32_t k = 0; k + 1 < p.sub_first.size(); ++k) {
        const uint32_t first = p.sub_first[k], end = p.sub_first[k + 1];
        for (uint32_t cls = 0; cls < jd::kClasses; ++cls)
            for (uint32_t form = 0; form < jd::kForms; ++form) {
                const uint32_t record0 = static_cast<uint32_t>(p.records.size());
                uint64_t tiles = 0;
                for (uint32_t i = first; i < end; ++i) {
                    const jh::File &f = b.files[i];
                    const uint32_t mine = (d_pixels + static_cast<uintptr_t>(b.images[i].offset)) % 16 == 0 ? jd::F_ALIGNED : jd::F_BYTES;
                    if (static_cast<uint32_t>(f.cls) != cls || mine != form || f.mcus_x == 0 || f.mcus_y == 0) continue;
                    jd::Record r;
                    std::memset(&r, 0, sizeof r);
                    for (uint32_t c = 0; c < f.ncomp; ++c) {
                        r.coef_at[c] = b.coef_at[i] - b.coef_at[first] + f.plane_at(c);
                        std::memcpy(r.q[c], f.q[f.comp[c].tq], sizeof r.q[c]);
                    }
                    r.out_at = b.images[i].offset;
                    r.width = f.width; r.height = f.height; r.mcus_x = f.mcus_x; r.mcus_y = f.mcus_y;
                    r.tiles_x = jd::tiles_x_of(f.mcus_x);
                    r.tiles = r.tiles_x * jd::tiles_y_of(f.mcus_y); // (at most 512 x 2048)
                    if (tiles + r.tiles > jd::kMaxTiles) return fail(PIXO_ERR_COMPRESSION, "Compression error: batch too large for one launch");
                    r.first_tile = static_cast<uint32_t>(tiles);
                    tiles += r.tiles;
                    p.records.push_back(r);
                    p.record_image.push_back(i);
                }
                if (p.records.size() > record0)
                    p.launches.push_back({k, cls, form, record0, static_cast<uint32_t>(p.records.size()) - record0, static_cast<uint32_t>(tiles)});
            }
    }
    return PIXO_OK;
}

// ---- PIXO_DECODE_DEVICE_ENTROPY ------------------------------------------------------------------------------------------------
struct EntropyLast { double device_ms = 0, build_ms = 0; uint32_t rounds = 0, files_device = 0, files_redone = 0; };
thread_local EntropyLast t_entropy_last; // (pixo_hip_debug_jpeg_entropy_last)

// Where a sub-batch's pieces lie in jd_states and jd_estatus
struct EntropyLayout {
    size_t entry, exit, border[2], count, first_block, states_bytes;
    size_t counters_bytes, status_bytes;
    EntropyLayout(uint64_t subs, uint64_t groups, uint64_t files)
    {
        size_t at = 0;
        entry = at; at += subs * 8;
        exit = at; at += subs * 8;
        border[0] = at; at += groups * 8;
        border[1] = at; at += groups * 8;
        count = at; at += subs * 4;
        first_block = at; at += subs * 4;
        states_bytes = std::max<size_t>(at, 16);
        counters_bytes = round16(8 * (je::kRoundCap + 2)); // two words a launch, at most kRoundCap + 2 launches
        status_bytes = counters_bytes + files * sizeof(je::FileStatus);
    }
};
int entropy_reserve(Context &c, uint64_t scan_bytes, uint64_t subs, uint64_t groups, uint64_t files)
{
    const EntropyLayout l(subs, groups, files);
    int rc;
    if ((rc = c.jd_hscan.reserve(std::max<uint64_t>(scan_bytes, 16))) || (rc = c.jd_scan.reserve(std::max<uint64_t>(scan_bytes, 16))) ||
        (rc = c.jd_states.reserve(l.states_bytes)) || (rc = c.jd_estatus.reserve(l.status_bytes)) || (rc = c.jd_hestatus.reserve(l.status_bytes)))
        return rc;
    return PIXO_OK;
}

// The device Huffman decode of files `dev` (indices into b.files, ascending, all of one sub-batch whose first file is `first`):
// records and scans up in one copy, the coefficients [0, coef_bytes) of jd_coef zeroed, the hand-over launches with a host wait
// for the counters behind each, verify / write / DC, the status records down and waited for: jd_hestatus holds them behind its
// counters, one per file of `dev`.  Everything was reserved by entropy_reserve.  cap: the round cap.
int entropy_on_device(Context &c, const DecodeBatch &b, const std::vector<uint32_t> &dev, uint32_t first, uint64_t coef_bytes, uint32_t cap, hipStream_t s,
                      EntropyLast &last)
{
    const uint32_t m = static_cast<uint32_t>(dev.size());
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t *up = c.jd_hscan.as<uint8_t>();
    je::FileRecord *records = reinterpret_cast<je::FileRecord *>(up);
    uint64_t scan_at = 0;
    uint32_t subs = 0, groups = 0;
    const size_t scans_from = m * sizeof(je::FileRecord);
    for (uint32_t n = 0; n < m; ++n) {
        const jh::File &f = b.files[dev[n]];
        je::FileRecord &r = records[n];
        je::fill_record(f, r);
        r.ecs_at = scan_at;
        for (uint32_t k = 0; k < f.ncomp; ++k) r.coef_at[k] += b.coef_at[dev[n]] - b.coef_at[first];
        r.first_sub = subs; r.first_group = groups; r.image = dev[n];
        const uint64_t padded = round16(f.ecs_len) + 16;
        std::memcpy(up + scans_from + scan_at, f.ecs, f.ecs_len);
        std::memset(up + scans_from + scan_at + f.ecs_len, 0, padded - f.ecs_len);
        scan_at += padded;
        subs += r.subs; groups += r.groups;
    }
    last.build_ms += ms_since(t0);
    const EntropyLayout l(subs, groups, m);
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    for (hipEvent_t &x : ev.e) HIP_TRY(hipEventCreate(&x));
    HIP_TRY(hipEventRecord(ev.e[0], s));
    HIP_TRY(hipMemcpyAsync(c.jd_scan.p, up, scans_from + scan_at, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(c.jd_estatus.p, 0, l.status_bytes, s));
    if (coef_bytes) HIP_TRY(hipMemsetAsync(c.jd_coef.p, 0, coef_bytes, s));
    HIP_TRY(hipEventRecord(c.jd_done, s));
    pixo_dev::JpegEntropyArgs a;
    uint8_t *states = c.jd_states.as<uint8_t>();
    a.records = c.jd_scan.as<je::FileRecord>(); a.files = m; a.groups = groups; a.subs = subs;
    a.scans = c.jd_scan.as<uint8_t>() + scans_from;
    a.entry = reinterpret_cast<je::State *>(states + l.entry); a.exit = reinterpret_cast<je::State *>(states + l.exit);
    a.border[0] = reinterpret_cast<je::State *>(states + l.border[0]); a.border[1] = reinterpret_cast<je::State *>(states + l.border[1]);
    a.count = reinterpret_cast<uint32_t *>(states + l.count); a.first_block = reinterpret_cast<uint32_t *>(states + l.first_block);
    a.counters = c.jd_estatus.as<uint32_t>();
    a.status = reinterpret_cast<je::FileStatus *>(c.jd_estatus.as<uint8_t>() + l.counters_bytes);
    a.coef = c.jd_coef.as<int16_t>();
    const uint32_t *counters = c.jd_hestatus.as<uint32_t>();
    for (uint32_t launch = 0; launch < je::kRoundCap + 2; ++launch) { // (a file that wants another launch uses a round of its cap in it)
        HIP_TRY(pixo_dev::launch_jpeg_entropy_sync(a, launch, cap, s));
        HIP_TRY(hipMemcpyAsync(c.jd_hestatus.as<uint32_t>() + 2 * launch, a.counters + 2 * launch, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(c.jd_done, s));
        HIP_TRY(hipEventSynchronize(c.jd_done)); // how many workgroups want another launch
        if (counters[2 * launch] == 0) break;
    }
    HIP_TRY(pixo_dev::launch_jpeg_entropy_finish(a, s));
    HIP_TRY(hipEventRecord(ev.e[1], s));
    HIP_TRY(hipMemcpyAsync(c.jd_hestatus.as<uint8_t>() + l.counters_bytes, a.status, m * sizeof(je::FileStatus), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(c.jd_done, s));
    HIP_TRY(hipEventSynchronize(c.jd_done));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    last.device_ms += ms;
    last.files_device += m;
    const je::FileStatus *status = reinterpret_cast<const je::FileStatus *>(c.jd_hestatus.as<uint8_t>() + l.counters_bytes);
    for (uint32_t n = 0; n < m; ++n) last.rounds = std::max(last.rounds, status[n].rounds);
    return PIXO_OK;
}

// The batch job with the Huffman decode on the device.  Per sub-batch: entropy_on_device over the files the plan sends there;
// then the host decodes, on the pool (or on the caller), what the device was not sent and what it does not vouch for, and
// decides in index order — the host's refusal is the call's —; those files' coefficients go up to their places; the decode
// launches follow as without the flag.  Every sub-batch waits on the host, so the pinned staging is free again for the next.
int decode_batch_device_entropy(Context &c, DecodeBatch &b, uint32_t flags, uint8_t *d_pixels, hipStream_t s, BatchLegs *legs)
{
    const uint32_t batch = static_cast<uint32_t>(b.files.size());
    int rc = await_last_job(c.jd_done);
    if (rc) return rc;
    t_entropy_last = EntropyLast();
    DecodePlan p;
    if ((rc = decode_plan(b, reinterpret_cast<uintptr_t>(d_pixels), flags, p))) return rc;
    const size_t record_bytes = p.records.size() * sizeof(jd::Record);
    if ((rc = c.jd_hrecords.reserve(std::max<size_t>(record_bytes, 16))) || (rc = c.jd_records.reserve(std::max<size_t>(record_bytes, 16))) ||
        (rc = c.jd_coef.reserve(std::max<uint64_t>(p.coef_bytes, 16))) || (rc = entropy_reserve(c, p.scan_bytes, p.subs, p.groups, p.device_files)))
        return rc;
    if (record_bytes) {
        std::memcpy(c.jd_hrecords.p, p.records.data(), record_bytes);
        HIP_TRY(hipMemcpyAsync(c.jd_records.p, c.jd_hrecords.p, record_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(c.jd_done, s));
    }
    b.threads = 1;
    size_t il = 0;
    for (uint32_t k = 0; k + 1 < p.sub_first.size(); ++k) {
        const uint32_t first = p.sub_first[k], end = p.sub_first[k + 1];
        const uint64_t coef_bytes = (end < batch ? b.coef_at[end] : b.staging) - b.coef_at[first];
        std::vector<uint32_t> dev, host;
        for (uint32_t i = first; i < end; ++i) (p.on_device[i] ? dev : host).push_back(i);
        if (!dev.empty()) {
            note_route(route::JPEG_ENTROPY_DEVICE);
            if ((rc = entropy_on_device(c, b, dev, first, coef_bytes, je::kRoundCap, s, t_entropy_last))) return rc;
            const je::FileStatus *status = reinterpret_cast<const je::FileStatus *>(c.jd_hestatus.as<uint8_t>() + EntropyLayout(0, 0, 0).counters_bytes);
            for (size_t n = 0; n < dev.size(); ++n)
                if (!status[n].vouched) {
                    host.push_back(dev[n]);
                    ++t_entropy_last.files_redone;
                    note_route(route::JPEG_ENTROPY_HOST_REDO);
                }
            std::sort(host.begin(), host.end());
        } else {
            HIP_TRY(hipEventRecord(c.jd_done, s));
            HIP_TRY(hipEventSynchronize(c.jd_done)); // (the staging below may still be going up for the sub-batch before)
        }
        // the host's files: decoded into the pinned staging one behind the other, in index order
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint64_t> host_at(host.size());
        uint64_t host_bytes = 0;
        for (size_t n = 0; n < host.size(); ++n) { host_at[n] = host_bytes; host_bytes += b.files[host[n]].coef_bytes(); }
        std::vector<jh::Kind> kind(host.size(), jh::OK);
        std::vector<std::string> msg(host.size());
        if (!host.empty()) {
            if ((rc = c.jd_hcoef.reserve(std::max<uint64_t>(host_bytes, 16)))) return rc;
            const uint32_t threads = (flags & PIXO_DECODE_ONE_THREAD) ? 1u : std::min<uint32_t>(static_cast<uint32_t>(host.size()), kDecodeBatchThreads);
            b.threads = std::max(b.threads, threads);
            std::atomic<uint32_t> next{0};
            run_on_threads(threads, [&](unsigned) {
                for (uint32_t n; (n = next.fetch_add(1, std::memory_order_relaxed)) < host.size();)
                    kind[n] = jh::entropy_decode(b.files[host[n]], reinterpret_cast<int16_t *>(c.jd_hcoef.as<uint8_t>() + host_at[n]), &msg[n]);
            });
        }
        b.entropy_ms += ms_since(t0) + t_entropy_last.build_ms; // the host's share: the records and scans laid out, the decodes
        t_entropy_last.build_ms = 0;
        for (size_t n = 0; n < host.size(); ++n)
            if ((rc = status_of(kind[n], msg[n], b.where(host[n])))) return rc;
        if (legs && (rc = legs->mark(s))) return rc;
        for (size_t n = 0; n < host.size(); ++n)
            if (const uint64_t bytes = b.files[host[n]].coef_bytes())
                HIP_TRY(hipMemcpyAsync(c.jd_coef.as<uint8_t>() + (b.coef_at[host[n]] - b.coef_at[first]), c.jd_hcoef.as<uint8_t>() + host_at[n], bytes,
                                       hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(c.jd_done, s));
        if (legs && (rc = legs->mark(s))) return rc;
        for (; il < p.launches.size() && p.launches[il].sub == k; ++il) {
            const DecodePlan::Launch &l = p.launches[il];
            HIP_TRY(pixo_dev::launch_jpeg_decode(c.jd_records.as<jd::Record>() + l.first_record, l.count, l.tiles, static_cast<int>(l.cls), static_cast<int>(l.form),
                                                 c.jd_coef.as<uint8_t>(), d_pixels, s));
        }
        if (legs && (rc = legs->mark(s))) return rc;
        HIP_TRY(hipEventRecord(c.jd_done, s));
    }
    return PIXO_OK;
}

// Everything behind phase 1: waits for this thread's previous JPEG decode job (the call's one host wait), decodes the scans into
// the pinned staging, then enqueues on `s`: all records in one copy; per sub-batch its coefficients in one copy and one launch
// per class and form present.  Nothing is enqueued after a refusal.
int decode_batch_on_device(Context &c, DecodeBatch &b, uint32_t flags, uint8_t *d_pixels, hipStream_t s, BatchLegs *legs = nullptr)
{
    if (flags & PIXO_DECODE_DEVICE_ENTROPY) return decode_batch_device_entropy(c, b, flags, d_pixels, s, legs);
    const uint32_t batch = static_cast<uint32_t>(b.files.size());
    int rc = await_last_job(c.jd_done); // (it reads jd_records and jd_coef, which go up from the pinned jd_hrecords and jd_hcoef)
    if (rc) return rc;
    if ((rc = c.jd_hcoef.reserve(std::max<uint64_t>(b.staging, 16)))) return rc;
    if ((rc = batch_entropy(b, c.jd_hcoef.as<uint8_t>(), flags))) return rc;
    DecodePlan p;
    if ((rc = decode_plan(b, reinterpret_cast<uintptr_t>(d_pixels), flags, p))) return rc;
    if (p.launches.empty()) return PIXO_OK; // (images without pixels only)
    // everything is reserved before any address is handed out
    const size_t record_bytes = p.records.size() * sizeof(jd::Record);
    if ((rc = c.jd_hrecords.reserve(record_bytes)) || (rc = c.jd_records.reserve(record_bytes)) || (rc = c.jd_coef.reserve(p.coef_bytes))) return rc;
    std::memcpy(c.jd_hrecords.p, p.records.data(), record_bytes);
    HIP_TRY(hipMemcpyAsync(c.jd_records.p, c.jd_hrecords.p, record_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c.jd_done, s)); // (until the job's own record: whatever has been enqueued when a later step fails)
    size_t il = 0;
    for (uint32_t k = 0; k + 1 < p.sub_first.size(); ++k) {
        const uint64_t from = b.coef_at[p.sub_first[k]];
        const uint64_t bytes = (p.sub_first[k + 1] < batch ? b.coef_at[p.sub_first[k + 1]] : b.staging) - from;
        if (legs && (rc = legs->mark(s))) return rc;
        if (bytes) HIP_TRY(hipMemcpyAsync(c.jd_coef.p, c.jd_hcoef.as<uint8_t>() + from, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(c.jd_done, s));
        if (legs && (rc = legs->mark(s))) return rc;
        for (; il < p.launches.size() && p.launches[il].sub == k; ++il) {
            const DecodePlan::Launch &l = p.launches[il];
            HIP_TRY(pixo_dev::launch_jpeg_decode(c.jd_records.as<jd::Record>() + l.first_record, l.count, l.tiles, static_cast<int>(l.cls), static_cast<int>(l.form),
                                                 c.jd_coef.as<uint8_t>(), d_pixels, s));
        }
        if (legs && (rc = legs->mark(s))) return rc;
        HIP_TRY(hipEventRecord(c.jd_done, s));
    }
    return PIXO_OK;
}

// Host files -> one block of the pinned pool the caller owns.  legs_ms: [0] entropy decode, [1] uploads, [2] kernels, [3] the copy down
int decode_batch_to_block(DecodeBatch &b, const pixo_png_file *files, uint32_t batch, uint32_t flags, uint8_t **out, size_t *out_len, pixo_png_image *images,
                          double *legs_ms)
{
    int rc = batch_walk(files, batch, b);
    if (rc) return rc;
    if (images) report(b.images, images);
    PIXO_THREAD_CONTEXT(c);
    const size_t n = static_cast<size_t>(b.total);
    if ((rc = reserve16(c.jd_out, std::max<size_t>(n, 16)))) return rc;
    BatchLegs legs;
    if ((rc = decode_batch_on_device(c, b, flags, c.jd_out.as<uint8_t>(), c.stream, legs_ms ? &legs : nullptr))) return rc;
    hipError_t e = hipSuccess;
    struct Down { // timed: events around the copy down
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Down() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } down;
    if (legs_ms) for (hipEvent_t &x : down.e) if ((e = hipEventCreate(&x)) != hipSuccess) return hip_fail(e, "jpeg decode");
    uint8_t *block = nullptr;
    size_t got = 0;
    if ((rc = download_pooled(c, c.jd_out.p, n, "jpeg decode", &block, &got, legs_ms ? down.e : nullptr))) return rc;
    if (legs_ms) {
        legs_ms[0] = b.entropy_ms;
        legs_ms[1] = legs_ms[2] = legs_ms[3] = 0;
        float ms = 0;
        for (size_t k = 0; k + 2 < legs.e.size() && e == hipSuccess; k += 3)
            for (int i = 0; i < 2 && e == hipSuccess; ++i) {
                e = hipEventElapsedTime(&ms, legs.e[k + i], legs.e[k + i + 1]);
                legs_ms[1 + i] += ms;
            }
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, down.e[0], down.e[1]);
        legs_ms[3] = ms;
        if (e != hipSuccess) { free_file(block); return hip_fail(e, "jpeg decode"); }
    }
    *out = block;
    *out_len = got;
    return PIXO_OK;
}

int batch_to_device(DecodeBatch &b, const pixo_png_file *files, uint32_t batch, uint32_t flags, void *d_pixels, size_t capacity, pixo_png_image *images, void *stream)
{
    int rc = batch_walk(files, batch, b);
    if (rc) return rc;
    report(b.images, images);
    if (capacity < b.total) return too_small(static_cast<size_t>(b.total));
    if (b.total) PIXO_REQUIRE(d_pixels);
    PIXO_CALLER_STREAM_CONTEXT(c, s, stream);
    return decode_batch_on_device(*c, b, flags, static_cast<uint8_t *>(d_pixels), s);
}

} // namespace

extern "C" {

int pixo_hip_jpeg_decode_batch_info(const pixo_png_file *files, uint32_t batch, pixo_png_image *images, size_t *total)
{
    int rc = batch_head(files, batch);
    if (rc) return rc;
    PIXO_REQUIRE(images);
    PIXO_REQUIRE(total);
    DecodeBatch b;
    if ((rc = batch_walk(files, batch, b))) return rc;
    report(b.images, images);
    *total = static_cast<size_t>(b.total);
    return PIXO_OK;
}

int pixo_hip_jpeg_decode_batch_device(const pixo_png_file *files, uint32_t batch, uint32_t flags, void *d_pixels, size_t capacity,
                                      pixo_png_image *images, void *stream)
{
    CallerStorageScope storage(d_pixels != nullptr && capacity != 0);
    const int rc = batch_head(files, batch);
    if (rc) return rc;
    PIXO_REQUIRE(images);
    DecodeBatch b;
    return batch_to_device(b, files, batch, flags, d_pixels, capacity, images, stream);
}

int pixo_hip_jpeg_decode_batch(const pixo_png_file *files, uint32_t batch, uint32_t flags, uint8_t **out, size_t *out_len, pixo_png_image *images)
{
    const int rc = batch_head(files, batch);
    if (rc) return rc;
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_len);
    PIXO_REQUIRE(images);
    DecodeBatch b;
    return decode_batch_to_block(b, files, batch, flags, out, out_len, images, nullptr);
}

int pixo_hip_debug_jpeg_decode_batch_plan(const pixo_png_file *files, uint32_t batch, uint32_t flags, uint32_t *sub_first, uint32_t *sub_count,
                                          uint8_t *classes, uint32_t *launches, uint32_t *threads)
{
    int rc = batch_head(files, batch);
    if (rc) return rc;
    PIXO_REQUIRE(sub_first);
    PIXO_REQUIRE(sub_count);
    PIXO_REQUIRE(classes);
    PIXO_REQUIRE(launches);
    PIXO_REQUIRE(threads);
    DecodeBatch b;
    if ((rc = batch_walk(files, batch, b))) return rc;
    DecodePlan p;
    if ((rc = decode_plan(b, 0, flags, p))) return rc;
    p.sub_first.report(sub_first, sub_count);
    for (uint32_t i = 0; i < batch; ++i) classes[i] = static_cast<uint8_t>(b.files[i].cls);
    *launches = static_cast<uint32_t>(p.launches.size());
    *threads = (flags & PIXO_DECODE_ONE_THREAD) ? 1u : std::min(batch, kDecodeBatchThreads);
    return PIXO_OK;
}

int pixo_hip_debug_jpeg_decode_batch_tables(const pixo_png_file *files, uint32_t batch, uint16_t *q)
{
    int rc = batch_head(files, batch);
    if (rc) return rc;
    PIXO_REQUIRE(q);
    DecodeBatch b;
    if ((rc = batch_walk(files, batch, b))) return rc;
    DecodePlan p;
    if ((rc = decode_plan(b, 0, 0, p))) return rc;
    std::memset(q, 0, static_cast<size_t>(batch) * sizeof p.records[0].q);
    for (size_t k = 0; k < p.records.size(); ++k) std::memcpy(q + static_cast<size_t>(p.record_image[k]) * 3 * 64, p.records[k].q, sizeof p.records[k].q);
    return PIXO_OK;
}

int pixo_hip_debug_jpeg_decode_batch_timed(const pixo_png_file *files, uint32_t batch, uint32_t flags, double ms[5])
{
    const int rc0 = batch_head(files, batch);
    if (rc0) return rc0;
    PIXO_REQUIRE(ms);
    uint8_t *block = nullptr;
    size_t n = 0;
    DecodeBatch b;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = decode_batch_to_block(b, files, batch, flags, &block, &n, nullptr, ms);
    if (rc) return rc;
    ms[4] = ms_since(t0);
    free_file(block);
    return PIXO_OK;
}

int pixo_hip_jpeg_decode(const uint8_t *file, size_t len, uint8_t **pixels, size_t *pixels_len, uint32_t *width, uint32_t *height, uint8_t *color_type)
{
    PIXO_REQUIRE(file);
    PIXO_REQUIRE(pixels);
    PIXO_REQUIRE(pixels_len);
    PIXO_REQUIRE(width);
    PIXO_REQUIRE(height);
    PIXO_REQUIRE(color_type);
    const pixo_png_file one = {file, len};
    pixo_png_image im;
    DecodeBatch b;
    b.single = true;
    const int rc = decode_batch_to_block(b, &one, 1, PIXO_DECODE_ONE_THREAD, pixels, pixels_len, &im, nullptr);
    if (rc) return rc;
    *width = im.width; *height = im.height; *color_type = im.color_type;
    return PIXO_OK;
}

int pixo_hip_jpeg_decode_info(const uint8_t *file, size_t len, uint32_t *width, uint32_t *height, uint8_t *color_type)
{
    PIXO_REQUIRE(file);
    PIXO_REQUIRE(width);
    PIXO_REQUIRE(height);
    PIXO_REQUIRE(color_type);
    const pixo_png_file one = {file, len};
    DecodeBatch b;
    b.single = true;
    const int rc = batch_walk(&one, 1, b);
    if (rc) return rc;
    *width = b.images[0].width; *height = b.images[0].height; *color_type = b.images[0].color_type;
    return PIXO_OK;
}

int pixo_hip_jpeg_decode_device(const uint8_t *file, size_t len, void *d_pixels, size_t capacity, uint32_t *width, uint32_t *height,
                                uint8_t *color_type, void *stream)
{
    CallerStorageScope storage(d_pixels != nullptr && capacity != 0);
    PIXO_REQUIRE(file);
    PIXO_REQUIRE(width);
    PIXO_REQUIRE(height);
    PIXO_REQUIRE(color_type);
    const pixo_png_file one = {file, len};
    pixo_png_image im;
    std::memset(&im, 0, sizeof im);
    DecodeBatch b;
    b.single = true;
    const int rc = batch_to_device(b, &one, 1, PIXO_DECODE_ONE_THREAD, d_pixels, capacity, &im, stream);
    if (!b.images.empty() && (rc == PIXO_OK || rc == PIXO_ERR_BUFFER_TOO_SMALL)) { *width = im.width; *height = im.height; *color_type = im.color_type; }
    return rc;
}

int pixo_hip_debug_jpeg_decode_coefficients(const uint8_t *file, size_t len, uint32_t component, int16_t *out, size_t capacity, uint32_t *blocks_w,
                                            uint32_t *blocks_h)
{
    PIXO_REQUIRE(file);
    PIXO_REQUIRE(blocks_w);
    PIXO_REQUIRE(blocks_h);
    jh::File f;
    std::string msg;
    int rc = status_of(jh::walk(file, len, f, &msg), msg, "");
    if (rc) return rc;
    if (component >= f.ncomp) return fail(PIXO_ERR_COMPRESSION, "Compression error: no such component");
    *blocks_w = f.blocks_w(component);
    *blocks_h = f.blocks_h(component);
    const uint64_t blocks = static_cast<uint64_t>(*blocks_w) * *blocks_h;
    if (capacity < blocks * 64) return too_small(static_cast<size_t>(blocks * 64 * sizeof(int16_t)));
    if (blocks) PIXO_REQUIRE(out);
    std::vector<int16_t> coef(static_cast<size_t>(f.coef_bytes() / 2));
    if ((rc = status_of(jh::entropy_decode(f, coef.data(), &msg), msg, ""))) return rc;
    const int16_t *plane = coef.data() + f.plane_at(component) / 2;
    for (uint64_t b = 0; b < blocks; ++b)
        for (uint32_t k = 0; k < 64; ++k) out[b * 64 + k] = plane[jd::coef_index(b, jh::kZigzag[k])];
    return PIXO_OK;
}

void pixo_hip_jpeg_entropy_geometry(uint32_t *sub_bytes, uint32_t *group_subs, uint32_t *round_cap, uint32_t *min_scan_bytes)
{
    if (sub_bytes) *sub_bytes = je::kSubBytes;
    if (group_subs) *group_subs = je::kGroupSubs;
    if (round_cap) *round_cap = je::kRoundCap;
    if (min_scan_bytes) *min_scan_bytes = je::kMinScanBytes;
}

int pixo_hip_debug_jpeg_entropy_plan(const pixo_png_file *files, uint32_t batch, uint32_t flags, uint8_t *on_device, uint32_t *sub_first, uint32_t *sub_count)
{
    int rc = batch_head(files, batch);
    if (rc) return rc;
    PIXO_REQUIRE(on_device);
    PIXO_REQUIRE(sub_first);
    PIXO_REQUIRE(sub_count);
    DecodeBatch b;
    if ((rc = batch_walk(files, batch, b))) return rc;
    DecodePlan p;
    if ((rc = decode_plan(b, 0, flags, p))) return rc;
    std::copy(p.on_device.begin(), p.on_device.end(), on_device);
    p.sub_first.report(sub_first, sub_count);
    return PIXO_OK;
}

int pixo_hip_debug_jpeg_entropy_batch(const pixo_png_file *files, uint32_t batch, uint32_t component, uint32_t round_cap, int16_t *out, const uint64_t *out_at,
                                      uint32_t *info)
{
    int rc = batch_head(files, batch);
    if (rc) return rc;
    PIXO_REQUIRE(out);
    PIXO_REQUIRE(out_at);
    PIXO_REQUIRE(info);
    if (round_cap > je::kRoundCap) return fail(PIXO_ERR_COMPRESSION, "Compression error: round cap above the library's");
    DecodeBatch b;
    if ((rc = batch_walk(files, batch, b))) return rc;
    PIXO_THREAD_CONTEXT(c);
    if ((rc = await_last_job(c.jd_done))) return rc;
    std::vector<uint32_t> dev;
    uint64_t scan_bytes = 0, subs = 0, groups = 0;
    for (uint32_t i = 0; i < batch; ++i) {
        info[4 * i] = 0; info[4 * i + 1] = 4; info[4 * i + 2] = info[4 * i + 3] = 0;
        if (!je::device_takes(b.files[i])) continue;
        dev.push_back(i);
        scan_bytes += scan_upload_bytes(b.files[i]);
        const uint32_t n = je::subs_of(static_cast<uint32_t>(b.files[i].ecs_len));
        subs += n; groups += je::groups_of(n);
    }
    if (dev.empty()) return PIXO_OK;
    if ((rc = c.jd_coef.reserve(std::max<uint64_t>(b.staging, 16))) || (rc = entropy_reserve(c, scan_bytes, subs, groups, dev.size()))) return rc;
    EntropyLast last;
    if ((rc = entropy_on_device(c, b, dev, 0, b.staging, round_cap ? round_cap : je::kRoundCap, c.stream, last))) return rc;
    std::vector<int16_t> coef(static_cast<size_t>(b.staging / 2));
    HIP_TRY(hipMemcpyAsync(coef.data(), c.jd_coef.p, b.staging, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    const je::FileStatus *status = reinterpret_cast<const je::FileStatus *>(c.jd_hestatus.as<uint8_t>() + EntropyLayout(0, 0, 0).counters_bytes);
    for (size_t n = 0; n < dev.size(); ++n) {
        const uint32_t i = dev[n];
        const jh::File &f = b.files[i];
        info[4 * i] = status[n].vouched; info[4 * i + 1] = status[n].why; info[4 * i + 2] = status[n].subs; info[4 * i + 3] = status[n].rounds;
        if (!status[n].vouched || component >= f.ncomp) continue;
        const int16_t *plane = coef.data() + (b.coef_at[i] + f.plane_at(component)) / 2;
        const uint64_t blocks = static_cast<uint64_t>(f.blocks_w(component)) * f.blocks_h(component);
        for (uint64_t k = 0; k < blocks; ++k)
            for (uint32_t z = 0; z < 64; ++z) out[out_at[i] + k * 64 + z] = plane[jd::coef_index(k, jh::kZigzag[z])];
    }
    return PIXO_OK;
}

void pixo_hip_debug_jpeg_entropy_last(double *device_ms, uint32_t *rounds, uint32_t *files_device, uint32_t *files_redone)
{
    if (device_ms) *device_ms = t_entropy_last.device_ms;
    if (rounds) *rounds = t_entropy_last.rounds;
    if (files_device) *files_device = t_entropy_last.files_device;
    if (files_redone) *files_redone = t_entropy_last.files_redone;
}

void pixo_hip_jpeg_decode_tile_mcus(uint32_t *mcus_x, uint32_t *mcus_y)
{
    if (mcus_x) *mcus_x = jd::kTileMcusX;
    if (mcus_y) *mcus_y = jd::kTileMcusY;
}

} // extern "C"
