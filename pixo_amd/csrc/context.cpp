// context.cpp — error state, per-device quantiser-table cache, the thread's execution context (HIP stream, grow-only
// device and pinned host buffers), the pool in which contexts outlive their threads, device selection, debug switches.
#include <algorithm>

#include "batch_steps.hpp"
#include "jpeg_kernels.hpp"
#include "jpeg_trellis.hpp"

namespace pixo_capi {

thread_local std::string t_error = "";

thread_local bool t_caller_storage = false;

int fail(int code, const std::string &msg)
{
    if (code == PIXO_ERR_BUFFER_TOO_SMALL && t_caller_storage) note_route(route::CALLER_RETRY);
    t_error = msg;
    return code;
}

int hip_fail(hipError_t e, const char *what)
{
    // pixo::Error::CompressionError(String) Display: "Compression error: {msg}"
    return fail(PIXO_ERR_COMPRESSION, std::string("Compression error: HIP ") + what + ": " +
                                          hipGetErrorString(e));
}

namespace {
std::mutex g_qt_mutex;
float *g_qt[kMaxDevices] = {};
thread_local hipStream_t t_producer = nullptr;
} // namespace

int device_tables(int device, const float **out)
{
    std::lock_guard<std::mutex> lock(g_qt_mutex);
    if (device < 0 || device >= kMaxDevices) return fail(PIXO_ERR_COMPRESSION, "Compression error: bad device index");
    if (!g_qt[device]) {
        std::vector<float> host(100 * pixo_host::kDeviceQtFloats);
        for (int q = 1; q <= 100; ++q) pixo_host::fill_device_qt(static_cast<uint8_t>(q), &host[(q - 1) * pixo_host::kDeviceQtFloats]);
        float *d = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), host.size() * sizeof(float)));
        HIP_TRY(hipMemcpy(d, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
        g_qt[device] = d;
    }
    *out = g_qt[device];
    return PIXO_OK;
}

// ---- debug switches ------------------------------------------------------------------------------------------------
namespace {
DebugSwitches parse_switches(const char *e)
{
    DebugSwitches v;
    if (!e) return v;
    const std::string all = e;
    for (size_t i = 0; i < all.size();) {
        size_t k = all.find(',', i);
        if (k == std::string::npos) k = all.size();
        const std::string item = all.substr(i, k - i);
        i = k + 1;
        const size_t eq = item.find('=');
        const std::string name = item.substr(0, eq), val = eq == std::string::npos ? "" : item.substr(eq + 1);
        const long num = val.empty() ? 0 : std::atol(val.c_str());
        if (name == "trace") v.trace = true;
        else if (name == "host_entropy") v.host_entropy = true;
        else if (name == "multipass_entropy") v.multipass_entropy = true;
        else if (name == "direct_stores") v.direct_stores = true;
        else if (name == "one_piece") v.one_piece = true;
        else if (name == "no_bands_upload") v.no_bands_upload = true;
        else if (name == "plain_host") v.plain_host = true;
        else if (name == "no_direct_small") v.no_direct_small = true;
        else if (name == "two_kernel_scan") v.two_kernel_scan = true;
        else if (name == "fused_batch") v.fused_batch = true;
        else if (name == "no_side_stats") v.no_side_stats = true;
        else if (name == "trellis_form") v.trellis_form = val == "lane" ? 1 : (val == "group" ? 2 : 0);
        else if (name == "coef_form") v.coef_form = val == "scalar" ? 1 : (val == "packed" ? 2 : 0);
        else if (name == "bands_upload_min_mb" && num > 0) v.bands_upload_min_mb = static_cast<uint32_t>(num);
        else if (name == "bands_upload_mb" && num > 0) v.bands_upload_mb = static_cast<uint32_t>(num);
        else if (name == "piece_groups" && num > 0) v.piece_groups = static_cast<uint64_t>(num);
        else if (name == "piece_medium") { v.piece_medium_forced = true; if (num > 0) v.piece_medium = static_cast<uint64_t>(num); }
        else if (name == "copy_threads") v.copy_threads = static_cast<unsigned>(num < 1 ? 1 : (num > 64 ? 64 : num));
        else if (name == "batch_parts" && num > 0) v.batch_parts = static_cast<uint32_t>(num);
        else if (name == "png_batch_bytes" && num > 0) v.png_batch_bytes = static_cast<uint64_t>(num);
        else if (name == "resize_batch_bytes" && num > 0) v.resize_batch_bytes = static_cast<uint64_t>(num);
        else if (name == "resize_images_rows" && num > 0) v.resize_images_rows = static_cast<uint32_t>(num > 65535 ? 65535 : num);
        else if (name == "convert_images_tiles" && num > 0) v.convert_images_tiles = static_cast<uint32_t>(num > 65536 ? 65536 : num);
        else if (name == "jpeg_images_blocks" && num > 0) v.jpeg_images_blocks = static_cast<uint64_t>(num);
        else if (name == "decode_batch_bytes" && num > 0) v.decode_batch_bytes = static_cast<uint64_t>(num);
        else if (name == "spin_budget" && !val.empty()) v.spin_budget = static_cast<uint32_t>(num < 0 ? 0 : num);
        else if (name == "piece_schedule") {
            std::vector<uint32_t> w;
            for (size_t p = 0; p < val.size();) {
                size_t q = val.find(':', p);
                if (q == std::string::npos) q = val.size();
                const long x = std::atol(val.substr(p, q - p).c_str());
                if (x > 0) w.push_back(static_cast<uint32_t>(x));
                p = q + 1;
            }
            if (!w.empty()) v.piece_schedule = w;
        } else if (!name.empty()) {
            std::fprintf(stderr, "[pixo_hip] PIXO_HIP_DEBUG: unknown switch '%s' ignored\n", name.c_str());
        }
    }
    return v;
}
DebugSwitches &switches()
{
    static DebugSwitches *d = [] {
        DebugSwitches *p = new DebugSwitches(parse_switches(std::getenv("PIXO_HIP_DEBUG")));
        pixo_dev::set_coef_form(p->coef_form);
        pixo_dev::set_trellis_form(p->trellis_form);
        return p;
    }();
    return *d;
}
} // namespace
const DebugSwitches &debug() { return switches(); }

// ---- grow-only buffers --------------------------------------------------------------------------------------------------
int Buf::regrow(size_t n)
{
    drop(); // (first: the old block's memory is free for the new one)
    size_t want = n;
    if (grow == Grow::Headroom) want = n + n / 4;
    else if (grow == Grow::SegEnds) want = (n / 8 + n / 32 + 16) * 8;
    const hipError_t e = mem == Mem::Device ? hipMalloc(&p, want) : hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess) { p = nullptr; return hip_fail(e, mem == Mem::Device ? "hipMalloc" : "hipHostMalloc"); }
    cap = want;
    return PIXO_OK;
}
void Buf::drop()
{
    if (p) (void)(mem == Mem::Device ? hipFree(p) : hipHostFree(p));
    p = nullptr; cap = 0; known = 0;
}

// ---- Context ---------------------------------------------------------------------------------------------------------
int Context::ensure()
{
    if (ready) return PIXO_OK;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(PIXO_ERR_COMPRESSION,
                    "Compression error: no MI355X/HIP device available (pixo_hip has no CPU fallback)");
    if (device < 0 || device >= n) return fail(PIXO_ERR_COMPRESSION, "Compression error: no HIP device " + std::to_string(device));
    DeviceScope on(device);
    if (on.err != hipSuccess) return hip_fail(on.err, "hipSetDevice");
    if (!mail) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&mail), sizeof(Mailbox), hipHostMallocDefault));
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    ready = true;
    return PIXO_OK;
}

namespace {
template <class F> void each_buf(Context &c, F &&f)
{
    Buf *bufs[] = {&c.d_px, &c.d_coef, &c.h_coef, &c.e_tables, &c.e_hist, &c.e_count, &c.e_len, &c.e_off, &c.e_tmp, &c.e_totals, &c.e_stream,
                   &c.e_tile_ff, &c.e_tile_base, &c.e_out, &c.e_seg_bytes, &c.e_seg_off, &c.e_code_state, &c.e_stuff_state, &c.e_pc_state,
                   &c.e_pc_spill, &c.e_chain, &c.e_seams, &c.e_segs, &c.h_segs, &c.p_in, &c.p_out, &c.p_sums, &c.p_scratch, &c.h_sums, &c.p_images, &c.h_images, &c.j_tables, &c.h_jtables, &c.j_out,
                   &c.q_work, &c.h_qwork, &c.q_index, &c.q_rows, &c.z_tok, &c.z_slots, &c.z_prev, &c.z_info, &c.z_stream, &c.z_crc, &c.h_zinfo,
                   &c.k_samples, &c.h_ksamples, &c.k_work, &c.h_kwork, &c.k_lut, &c.k_carry,
                   &c.t_raw, &c.t_trail, &c.t_plain, &c.g_flags, &c.g_rank, &c.g_by_rank, &c.h_file, &c.r_in, &c.r_out, &c.r_mid, &c.r_tables,
                   &c.r_stage, &c.rb_in, &c.rb_out, &c.rb_mid, &c.rb_tables, &c.rb_stage, &c.cv_in, &c.cv_out, &c.cv_records, &c.h_cv_records, &c.u_inflated, &c.u_stream, &c.u_rows, &c.u_out, &c.u_tables, &c.h_utables,
                   &c.h_zin, &c.u_zin, &c.u_zout, &c.h_zout, &c.h_uruns, &c.u_runs,
                   &c.jd_hcoef, &c.jd_coef, &c.jd_hrecords, &c.jd_records, &c.jd_out, &c.jd_hscan, &c.jd_scan, &c.jd_states, &c.jd_estatus, &c.jd_hestatus};
    for (Buf *b : bufs) f(*b);
}
} // namespace

size_t Context::held_bytes() const
{
    size_t n = 0;
    each_buf(const_cast<Context &>(*this), [&](Buf &b) { n += b.cap; });
    return n;
}

void Context::shrink_to(size_t max_buffer_bytes)
{ // (a live thread on the context's device; the stream is idle)
    if (!ready) return;
    DeviceScope on(device);
    if (on.err != hipSuccess) return;
    if (stream) (void)hipStreamSynchronize(stream);
    each_buf(*this, [&](Buf &b) { if (b.cap > max_buffer_bytes) b.drop(); });
}

void Context::release()
{
    if (helper) { destroy_copy_helper(helper); helper = nullptr; } // (stops and joins the context's second host thread)
    if (!ready) return;
    DeviceScope on(device);
    if (on.err != hipSuccess) return;
    if (stream) (void)hipStreamSynchronize(stream);
    each_buf(*this, [](Buf &b) { b.drop(); });
    if (mail) (void)hipHostFree(mail);
    mail = nullptr;
    if (stream) (void)hipStreamDestroy(stream);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (upload_stream) (void)hipStreamDestroy(upload_stream);
    copy_stream = upload_stream = nullptr;
    for (hipEvent_t e : piece_done) (void)hipEventDestroy(e);
    piece_done.clear();
    for (hipEvent_t e : band_up) (void)hipEventDestroy(e);
    band_up.clear();
    if (producer_done) (void)hipEventDestroy(producer_done);
    producer_done = nullptr;
    if (stats_done) (void)hipEventDestroy(stats_done);
    if (side_ready) (void)hipEventDestroy(side_ready);
    stats_done = side_ready = nullptr;
    if (r_done) (void)hipEventDestroy(r_done);
    r_done = nullptr;
    if (rb_done) (void)hipEventDestroy(rb_done);
    rb_done = nullptr;
    if (cv_done) (void)hipEventDestroy(cv_done);
    cv_done = nullptr;
    if (u_done) (void)hipEventDestroy(u_done);
    u_done = nullptr;
    if (jd_done) (void)hipEventDestroy(jd_done);
    jd_done = nullptr;
    stream = nullptr; ready = false;
}

// Contexts outlive the threads that use them.  A thread's context must not be torn down by a
// thread-local destructor: those run when the HIP runtime's own per-thread state may already be gone
// (it was created later, so it is destroyed earlier), and — for threads still winding down while main()
// returns — concurrently with the runtime's atexit teardown; hipFree / hipHostFree from there crashed
// (SIGSEGV in amd::Context::svmFree with 16 threads ending at once, profiles/r02_thread_exit_crash.txt).
// So a thread that ends only parks its context here (a mutex and a vector push, no HIP call); the next
// thread that needs one adopts it — buffers, stream and all, which also spares a server with a thread per
// request every hipMalloc.  What is parked is bounded by BYTES as well as by count: after one 16384x16384 image a
// context holds ~2 GB of HBM and ~0.4 GB of pinned host memory, and a server with a thread per request would park
// sixteen of those.  Live threads enforce the bound when they take a context (the oldest parked contexts first give up
// their large buffers, then go entirely); pixo_hip_trim() releases everything.  A context of another device is never
// re-bound on the adopting thread's hot path: a thread that finds none of its own device makes a new one.  Nothing is
// destroyed at process exit (the pool is leaked on purpose).
constexpr size_t kIdleContextsKept = 16;
constexpr size_t kIdleBytesKept = size_t{8} << 30;    // device + pinned bytes all parked contexts together may keep (3 % of the 288 GB; round 6: with
                                                      // 1 GiB four parked contexts of 4096x4096 files shrank — hipFree, a device-wide synchronisation each —
                                                      // under the feet of the threads that took them over: 217 -> 650-917 us per file, tools/mt_device_files.py)
constexpr size_t kIdleBufferKept = size_t{64} << 20;  // a parked context that must shrink keeps buffers up to this size
Context *ContextPool::take(int device)
{
    std::vector<Context *> excess, shrink;
    Context *c = nullptr;
    {
        std::lock_guard<std::mutex> lock(m);
        for (size_t i = idle.size(); i-- > 0;)
            if (idle[i]->device == device) { c = idle[i]; idle.erase(idle.begin() + static_cast<long>(i)); break; }
        while (idle.size() > kIdleContextsKept) { excess.push_back(idle.front()); idle.erase(idle.begin()); }
        size_t bytes = 0;
        for (Context *x : idle) bytes += x->held_bytes();
        for (size_t i = 0; i < idle.size() && bytes > kIdleBytesKept;) { // oldest first
            Context *x = idle[i];
            bytes -= x->held_bytes();
            idle.erase(idle.begin() + static_cast<long>(i));
            shrink.push_back(x);
        }
    }
    for (Context *x : excess) { x->release(); delete x; } // (a live thread: HIP calls are fine here)
    for (Context *x : shrink) {
        x->shrink_to(kIdleBufferKept);
        give(x); // (back at the young end: small now)
    }
    if (!c) { c = new Context; c->device = device; }
    return c;
}
void ContextPool::give(Context *c) // no HIP calls: may run in a thread-local destructor
{
    std::lock_guard<std::mutex> lock(m);
    idle.push_back(c);
}
void ContextPool::drain() // frees every parked context (pixo_hip_trim)
{
    std::vector<Context *> all;
    {
        std::lock_guard<std::mutex> lock(m);
        all.swap(idle);
    }
    for (Context *x : all) { x->release(); delete x; }
}
ContextPool &pool()
{
    static ContextPool *p = new ContextPool;
    return *p;
}
ThreadSlot::~ThreadSlot() { if (c) pool().give(c); }
thread_local ThreadSlot t_slot;
Context &thread_context()
{
    if (!t_slot.c) t_slot.c = pool().take(t_slot.device);
    return *t_slot.c;
}

// Device-pointer entry points run on the context's own stream.  What the caller enqueued before the call
// — on the stream it named with pixo_hip_set_producer_stream, by default the NULL stream — is ordered
// in front of it with an event (no host synchronisation).
int order_after_producer(Context &c)
{
    if (!c.producer_done) HIP_TRY(hipEventCreateWithFlags(&c.producer_done, hipEventDisableTiming));
    if (hipEventRecord(c.producer_done, t_producer) != hipSuccess) {
        // the named stream is not one of this context's device (a stale setting from work on another GPU): an event of
        // this device cannot be recorded on it — wait for that stream on the host instead of failing the call
        (void)hipGetLastError();
        HIP_TRY(hipStreamSynchronize(t_producer));
        return PIXO_OK;
    }
    HIP_TRY(hipStreamWaitEvent(c.stream, c.producer_done, 0));
    return PIXO_OK;
}

// binds the thread's context to the HIP device that is current for the caller
int context_on_current_device(Context **out)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (t_slot.device != dev) (void)pixo_hip_set_device(dev);
    Context &c = thread_context();
    int rc = c.ensure();
    if (rc) return rc;
    if ((rc = order_after_producer(c))) return rc;
    *out = &c;
    return PIXO_OK;
}

// ---- the batch drivers' shared steps (batch_steps.hpp) -----------------------------------------------------------------
int caller_stream_context(void *stream, Context **c, hipStream_t *s)
{
    if (const int rc = context_on_current_device(c)) return rc; // (records the producer stream's event)
    *s = static_cast<hipStream_t>(stream);
    if ((*c)->producer_done) HIP_TRY(hipStreamWaitEvent(*s, (*c)->producer_done, 0));
    return PIXO_OK;
}

int await_last_job(hipEvent_t &fence)
{
    if (!fence) HIP_TRY(hipEventCreateWithFlags(&fence, hipEventDisableTiming));
    // The job before this one on the context may still be reading the tables and records, and its pinned staging may still be on
    // its way up: this job is about to overwrite both.  It is the call's only host wait — everything behind it is enqueued — and it
    // waits for the job before, not for the stream: what the caller enqueued since is not waited for.
    HIP_TRY(hipEventSynchronize(fence));
    return PIXO_OK;
}

int bad_color_type(uint8_t ct, const std::string &where)
{
    return fail(PIXO_ERR_INVALID_COLOR_ARG, "Invalid color type: " + std::to_string(ct) + ". Expected 0 (Gray), 1 (GrayAlpha), 2 (Rgb), or 3 (Rgba)" + where);
}

int record_extent(uint64_t offset, uint64_t bytes, const char *what, const std::string &where, uint64_t *furthest)
{
    const uint64_t most = uint64_t{1} << 62;
    if (offset > most || offset + bytes > most) return fail(PIXO_ERR_COMPRESSION, std::string("Compression error: batch ") + what + " too large" + where);
    *furthest = std::max(*furthest, offset + bytes);
    return PIXO_OK;
}

} // namespace pixo_capi

using namespace pixo_capi;

extern "C" {

int pixo_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pixo_hip_set_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
        return fail(PIXO_ERR_COMPRESSION, "Compression error: no HIP device " + std::to_string(device));
    if (t_slot.c && t_slot.c->device != device) { // rebind: park the old device's context, adopt one of the new device
        pool().give(t_slot.c);
        t_slot.c = nullptr;
    }
    t_slot.device = device;
    return PIXO_OK;
}

int pixo_hip_set_producer_stream(void *stream)
{
    t_producer = static_cast<hipStream_t>(stream);
    return PIXO_OK;
}

void *pixo_hip_get_producer_stream(void) { return t_producer; }

int pixo_hip_debug_configure(const char *switches_or_null)
{ // tests and tools only; not synchronised with calls in flight on other threads
    switches() = parse_switches(switches_or_null ? switches_or_null : std::getenv("PIXO_HIP_DEBUG"));
    pixo_dev::set_coef_form(switches().coef_form);
    pixo_dev::set_trellis_form(switches().trellis_form);
    return PIXO_OK;
}

int pixo_hip_trim(void)
{
    if (t_slot.c) t_slot.c->release();
    pool().drain();
    drop_kept_blocks();
    drop_batch_worker_buffers();
    return PIXO_OK;
}

void pixo_hip_free(void *p) { free_file(p); }
void pixo_hip_copy_file(void *dst, const void *src, size_t n)
{
    if (dst && src && n) big_copy(static_cast<uint8_t *>(dst), static_cast<const uint8_t *>(src), n);
}

const char *pixo_hip_last_error(void) { return t_error.c_str(); }

const char *pixo_hip_version(void) { return "pixo_hip 0.4.0 (gfx950; reference pixo 0.4.1)"; }

} // extern "C"
