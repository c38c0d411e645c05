// png_quantize_api.cpp — PNG lossy mode: the gate, the histogram and median cut on the host, k-means, the 64^3 table, the
// mapping and the dither on the device (png_quantize.hip); the extern "C" quantize entry points.  Reference:
// src/png/mod.rs:469-511 (gate and call), :1160-1339 (median cut), :1346-1390 (k-means), :1505-1762 (quantize_image,
// should_quantize_auto).  The one stated departure: above 8,192 sampled colours the reference keeps the 8,192 most frequent by
// an UNSTABLE sort, which does not say which of several equally frequent colours stay; here ties go to the smaller key.
#include "capi_internal.hpp"
#include "png_quantize.hpp"

#include <algorithm>
#include <atomic>
#include <vector>

using namespace pixo_capi;
using namespace pixo_pngq;

namespace {

constexpr size_t kGateSamples = 20000, kHistSamples = 50000, kMaxHistColors = 8192;

// How the dither ran in this process (tests, tools: pixo_hip_debug_png_dither_stats): chained launches, calls served band by
// band, chained launches that gave up waiting (each also counts as a look-back fallback and notes route::FALLBACK).
std::atomic<uint64_t> g_dither_chained{0}, g_dither_banded{0}, g_dither_gave_up{0};

struct ColorCount { uint32_t key, count; };
inline uint32_t chan(uint32_t key, int c) { return (key >> (24 - 8 * c)) & 255u; }

// Everything small the quantiser exchanges with the host, the same layout on both sides.
struct QuantWork {
    unsigned long long acc[kMaxPalette * 5]; // a k-means round's sums
    uint32_t colors[kMaxHistColors], counts[kMaxHistColors];
    uint32_t palette[kMaxPalette];
    uint32_t state[pixo_dev::kDitherStateWords];
};

// ---- median cut (mod.rs:1160-1339, without the k-means that follows it there) ----------------------------------------
struct ColorBox {
    std::vector<ColorCount> colors;
    uint8_t lo[4], hi[4];
    explicit ColorBox(std::vector<ColorCount> cs) : colors(std::move(cs))
    {
        for (int c = 0; c < 4; ++c) { lo[c] = 255; hi[c] = 0; }
        for (const ColorCount &cc : colors)
            for (int c = 0; c < 4; ++c) {
                lo[c] = std::min<uint8_t>(lo[c], static_cast<uint8_t>(chan(cc.key, c)));
                hi[c] = std::max<uint8_t>(hi[c], static_cast<uint8_t>(chan(cc.key, c)));
            }
    }
    void range(int *channel, uint32_t *score) const // :1211-1238: 2 R, 4 G, 1 B, 3 A; only a strictly greater score wins
    {
        static const uint32_t weight[4] = {2, 4, 1, 3};
        *channel = 0;
        *score = static_cast<uint32_t>(hi[0] - lo[0]) * weight[0];
        for (int c = 1; c < 4; ++c) {
            const uint32_t s = static_cast<uint32_t>(hi[c] - lo[c]) * weight[c];
            if (s > *score) { *score = s; *channel = c; }
        }
    }
    uint32_t entry() const // :1274-1298: the floor of the weighted mean
    {
        uint64_t sum[4] = {0, 0, 0, 0}, total = 0;
        for (const ColorCount &cc : colors) {
            for (int c = 0; c < 4; ++c) sum[c] += static_cast<uint64_t>(chan(cc.key, c)) * cc.count;
            total += cc.count;
        }
        if (total == 0) return 255u;
        return (static_cast<uint32_t>(sum[0] / total) << 24) | (static_cast<uint32_t>(sum[1] / total) << 16) | (static_cast<uint32_t>(sum[2] / total) << 8) |
               static_cast<uint32_t>(sum[3] / total);
    }
};

std::vector<uint32_t> median_cut(const std::vector<ColorCount> &colors, uint32_t max_colors)
{
    if (colors.empty()) return {255u};
    std::vector<ColorBox> boxes;
    boxes.emplace_back(colors);
    while (boxes.size() < max_colors) {
        size_t idx = 0; // max_by_key keeps the LAST maximum
        uint32_t best = 0;
        for (size_t i = 0; i < boxes.size(); ++i) {
            int ch;
            uint32_t s;
            boxes[i].range(&ch, &s);
            if (i == 0 || s >= best) { best = s; idx = i; }
        }
        if (boxes[idx].colors.size() <= 1) break;
        ColorBox b = std::move(boxes[idx]);
        boxes.erase(boxes.begin() + static_cast<long>(idx));
        int ch;
        uint32_t s;
        b.range(&ch, &s);
        std::stable_sort(b.colors.begin(), b.colors.end(), [ch](const ColorCount &x, const ColorCount &y) { return chan(x.key, ch) < chan(y.key, ch); });
        uint32_t total = 0, acc = 0; // u32 like the reference's (sampled counts stay far below 2^32)
        for (const ColorCount &cc : b.colors) total += cc.count;
        size_t split = 0;
        for (size_t i = 0; i < b.colors.size(); ++i) {
            acc += b.colors[i].count;
            if (acc >= total / 2) { split = i; break; }
        }
        split = std::min(split, b.colors.size() - 2);
        boxes.emplace_back(std::vector<ColorCount>(b.colors.begin(), b.colors.begin() + static_cast<long>(split) + 1));
        boxes.emplace_back(std::vector<ColorCount>(b.colors.begin() + static_cast<long>(split) + 1, b.colors.end()));
    }
    std::vector<uint32_t> palette;
    for (const ColorBox &b : boxes) palette.push_back(b.entry());
    return palette;
}

// keys (any order; sorted here) -> (colour, count) runs, each sample standing for `stride` pixels (:1540-1580)
std::vector<ColorCount> histogram(uint32_t *keys, size_t n, uint64_t stride)
{
    std::sort(keys, keys + n);
    const uint32_t step = static_cast<uint32_t>(stride);
    std::vector<ColorCount> colors;
    for (size_t i = 0; i < n;) {
        size_t j = i;
        uint64_t count = 0;
        while (j < n && keys[j] == keys[i]) { count = std::min<uint64_t>(count + step, 0xFFFFFFFFull); ++j; }
        colors.push_back({keys[i], static_cast<uint32_t>(count)});
        i = j;
    }
    if (colors.size() > kMaxHistColors) { // the most frequent; ties: the smaller key (the departure named at the top)
        std::sort(colors.begin(), colors.end(), [](const ColorCount &x, const ColorCount &y) { return x.count != y.count ? x.count > y.count : x.key < y.key; });
        colors.resize(kMaxHistColors);
    }
    return colors;
}

bool gate_passes(uint32_t *keys, size_t n, uint32_t max_colors) // should_quantize_auto's verdict on its samples (:1742-1761)
{
    if (n == 0) return false;
    std::sort(keys, keys + n);
    const size_t unique = static_cast<size_t>(std::unique(keys, keys + n) - keys), threshold = static_cast<size_t>(max_colors) * 32;
    return unique > max_colors && unique <= threshold;
}

inline uint64_t samples_of(uint64_t pixels, uint64_t stride) { return (pixels + stride - 1) / stride; }

struct StageClock {
    bool on = debug().trace;
    hipStream_t stream;
    hipEvent_t from = nullptr, to = nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    explicit StageClock(hipStream_t s) : stream(s)
    {
        if (!on) return;
        on = hipEventCreate(&from) == hipSuccess && hipEventCreate(&to) == hipSuccess && hipEventRecord(from, stream) == hipSuccess;
    }
    ~StageClock()
    {
        if (from) (void)hipEventDestroy(from);
        if (to) (void)hipEventDestroy(to);
    }
    StageClock(const StageClock &) = delete;
    StageClock &operator=(const StageClock &) = delete;
    void lap(const char *what)
    {
        if (!on) return;
        float device_ms = 0;
        if (hipEventRecord(to, stream) != hipSuccess || hipEventSynchronize(to) != hipSuccess || hipEventElapsedTime(&device_ms, from, to) != hipSuccess) { on = false; return; }
        const auto n = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[pixo_hip] %-28s %8.3f ms   device events %8.3f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count(), device_ms);
        std::swap(from, to);
        (void)hipEventRecord(from, stream);
        t = std::chrono::steady_clock::now();
    }
};

void palette_out_of(const pixo_png_layout &layout, uint8_t (*palette_out)[4], uint32_t *palette_len, uint32_t *trns_len, uint32_t trns)
{
    std::memcpy(palette_out, layout.palette, sizeof(layout.palette[0]) * layout.palette_len);
    *palette_len = layout.palette_len;
    *trns_len = trns;
}

} // namespace

int pixo_capi::png_check_quantization(const pixo_png_quantization *quantization)
{
    PIXO_REQUIRE(quantization);
    if (quantization->mode > PIXO_PNG_QUANT_FORCE) return fail(PIXO_ERR_COMPRESSION, "Compression error: unknown PNG quantization mode");
    return PIXO_OK;
}

int pixo_capi::png_quantize_on_device(Context &c, const void *d_px, const pixo_png_options &o, const pixo_png_quantization &q, bool *applied,
                                      pixo_png_layout *layout, uint32_t *trns_len)
{
    *applied = false;
    const bool colour = o.color_type == PIXO_RGB || o.color_type == PIXO_RGBA;
    if (q.mode == PIXO_PNG_QUANT_OFF || !colour) return PIXO_OK; // mod.rs:470-481
    const uint32_t spp = bytes_per_pixel(o.color_type), max_colors = std::min<uint32_t>(q.max_colors, kMaxPalette);
    const uint64_t pixels = static_cast<uint64_t>(o.width) * o.height;
    // Debug switch `trace`: per stage, the time between two events on the context's stream (what the device spent) and the
    // host's wall time (launches, copies and the host's own work included).
    StageClock watch(c.stream);
    auto lap = [&](const char *what) { watch.lap(what); };

    // Both sets of samples in one buffer, one copy down (one set where the strides agree)
    const bool gate = q.mode == PIXO_PNG_QUANT_AUTO;
    const uint64_t stride_h = std::max<uint64_t>(pixels / kHistSamples, 1), stride_g = std::max<uint64_t>(pixels / kGateSamples, 1);
    const bool own_gate_samples = gate && stride_g != stride_h;
    const uint32_t count_h = static_cast<uint32_t>(samples_of(pixels, stride_h)), count_g = own_gate_samples ? static_cast<uint32_t>(samples_of(pixels, stride_g)) : 0;
    const size_t sample_bytes = (static_cast<size_t>(count_h) + count_g) * sizeof(uint32_t);
    int rc;
    // (the host side has room for a second copy of the histogram's samples: the gate sorts its own when it shares them)
    if ((rc = c.k_samples.reserve(sample_bytes)) || (rc = c.h_ksamples.reserve(sample_bytes + count_h * sizeof(uint32_t))) ||
        (rc = c.k_work.reserve(sizeof(QuantWork))) || (rc = c.h_kwork.reserve(sizeof(QuantWork))) || (rc = c.k_lut.reserve(kLutCells)) ||
        (rc = reserve16(c.q_index, pixels)))
        return rc;
    uint32_t *keys = c.h_ksamples.as<uint32_t>();
    HIP_TRY(pixo_dev::launch_pngq_gather(d_px, spp, stride_h, count_h, stride_g, count_g, c.k_samples.as<uint32_t>(), c.stream));
    HIP_TRY(hipMemcpyAsync(keys, c.k_samples.p, sample_bytes, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    lap("png quantize: gather");
    if (gate) {
        uint32_t *gate_keys = keys + count_h;
        size_t gate_n = count_g;
        if (!own_gate_samples) { // the histogram's samples are the gate's: judged on a copy
            gate_n = count_h;
            std::memcpy(gate_keys, keys, gate_n * sizeof(uint32_t));
        }
        if (!gate_passes(gate_keys, gate_n, max_colors)) { lap("png quantize: host part"); return PIXO_OK; }
    }
    const std::vector<ColorCount> colors = histogram(keys, count_h, stride_h);
    QuantWork *host = c.h_kwork.as<QuantWork>(), *dev = c.k_work.as<QuantWork>();
    std::vector<uint32_t> palette;
    const bool early_out = colors.size() <= max_colors; // :1583-1614: the sorted colours are the palette
    if (early_out) {
        for (const ColorCount &cc : colors) palette.push_back(cc.key);
    } else {
        palette = median_cut(colors, max_colors);
    }
    const uint32_t n = static_cast<uint32_t>(palette.size());
    if (n == 0 || n > kMaxPalette) return fail(PIXO_ERR_COMPRESSION, "Compression error: the quantiser's palette is inconsistent");
    std::copy(palette.begin(), palette.end(), host->palette);
    lap("png quantize: host part");
    if (!early_out) {
        for (size_t i = 0; i < colors.size(); ++i) { host->colors[i] = colors[i].key; host->counts[i] = colors[i].count; }
        HIP_TRY(hipMemcpyAsync(dev->colors, host->colors, colors.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipMemcpyAsync(dev->counts, host->counts, colors.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
        for (int round = 0; round < 2; ++round) { // refine_palette_kmeans: the centroid is the floor of the weighted mean; empty clusters stay
            HIP_TRY(hipMemcpyAsync(dev->palette, host->palette, n * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
            HIP_TRY(pixo_dev::launch_pngq_assign(dev->colors, dev->counts, static_cast<uint32_t>(colors.size()), dev->palette, n, dev->acc, c.stream));
            HIP_TRY(hipMemcpyAsync(host->acc, dev->acc, static_cast<size_t>(n) * 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
            HIP_TRY(hipStreamSynchronize(c.stream));
            for (uint32_t i = 0; i < n; ++i) {
                const unsigned long long *a = host->acc + 5 * i;
                if (a[4]) host->palette[i] = (static_cast<uint32_t>(a[0] / a[4]) << 24) | (static_cast<uint32_t>(a[1] / a[4]) << 16) | (static_cast<uint32_t>(a[2] / a[4]) << 8) | static_cast<uint32_t>(a[3] / a[4]);
            }
        }
        lap("png quantize: k-means");
    }
    HIP_TRY(hipMemcpyAsync(dev->palette, host->palette, n * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
    if (!early_out) {
        HIP_TRY(pixo_dev::launch_pngq_lut(dev->palette, n, c.k_lut.as<uint8_t>(), c.stream));
        lap("png quantize: LUT");
    }
    if (early_out || !q.dithering) {
        HIP_TRY(pixo_dev::launch_pngq_map(d_px, pixels, spp, early_out ? nullptr : c.k_lut.as<uint8_t>(), dev->palette, n, c.q_index.as<uint8_t>(), c.stream));
        lap("png quantize: map");
    } else {
        const uint32_t bands = (o.height + kBandRows - 1) / kBandRows;
        if ((rc = c.k_carry.reserve(static_cast<size_t>(bands) * o.width * sizeof(unsigned long long)))) return rc;
        const pixo_dev::DitherArgs a{static_cast<const uint8_t *>(d_px), spp, o.width, o.height, c.k_lut.as<uint8_t>(), dev->palette, n,
                                     c.q_index.as<uint8_t>(), c.k_carry.as<unsigned long long>(), dev->state};
        bool band_by_band = debug().spin_budget == 0 || bands == 1; // (tests force the second form with spin_budget=0)
        if (!band_by_band) {
            g_dither_chained.fetch_add(1, std::memory_order_relaxed);
            HIP_TRY(pixo_dev::launch_pngq_dither_chained(a, debug().spin_budget, c.stream));
            HIP_TRY(hipMemcpyAsync(host->state, dev->state, sizeof(host->state), hipMemcpyDeviceToHost, c.stream));
            HIP_TRY(hipStreamSynchronize(c.stream));
            band_by_band = host->state[1] != 0; // a band gave up waiting: nothing of the launch is kept
            if (band_by_band) {
                g_dither_gave_up.fetch_add(1, std::memory_order_relaxed);
                note_lookback_fallback();
                lap("png quantize: dither gave up");
            }
        }
        if (band_by_band) {
            g_dither_banded.fetch_add(1, std::memory_order_relaxed);
            for (uint32_t b = 0; b < bands; ++b) HIP_TRY(pixo_dev::launch_pngq_dither_band(a, b, c.stream));
            HIP_TRY(hipMemcpyAsync(host->state, dev->state, sizeof(host->state), hipMemcpyDeviceToHost, c.stream));
            HIP_TRY(hipStreamSynchronize(c.stream));
            if (host->state[1]) return fail(PIXO_ERR_COMPRESSION, "Compression error: a dither band read a column the band above had not written");
        }
        lap("png quantize: dither");
    }

    std::memset(layout, 0, sizeof(*layout));
    layout->color_type_byte = 3;
    layout->bit_depth = 8;
    layout->bytes_per_pixel = 1;
    layout->row_bytes = o.width;
    layout->palette_len = n;
    *trns_len = 0; // maybe_trim_transparency (:1888-1902): up to the last alpha that is not 255
    for (uint32_t i = 0; i < n; ++i) {
        for (int ch = 0; ch < 4; ++ch) layout->palette[i][ch] = static_cast<uint8_t>(chan(host->palette[i], ch));
        if ((host->palette[i] & 255u) != 255u) *trns_len = i + 1;
    }
    layout->has_trns = *trns_len ? 1 : 0;
    *applied = true;
    return PIXO_OK;
}

extern "C" {

int pixo_hip_png_quantize(const uint8_t *data, size_t data_len, const pixo_png_options *options, const pixo_png_quantization *quantization,
                          uint8_t *indices_out, size_t indices_capacity, uint8_t (*palette_out)[4], uint32_t *palette_len, uint32_t *trns_len,
                          uint8_t *applied)
{
    int rc = png_check_options(options, true, data_len);
    if (rc) return rc;
    PIXO_REQUIRE(data);
    if ((rc = png_check_quantization(quantization))) return rc;
    PIXO_REQUIRE(palette_out);
    PIXO_REQUIRE(palette_len);
    PIXO_REQUIRE(trns_len);
    PIXO_REQUIRE(applied);
    PIXO_THREAD_CONTEXT(c);
    if ((rc = upload(c, c.p_in, data, data_len))) return rc;
    bool did = false;
    pixo_png_layout layout;
    uint32_t trns = 0;
    if ((rc = png_quantize_on_device(c, c.p_in.p, *options, *quantization, &did, &layout, &trns))) return rc;
    *applied = did ? 1 : 0;
    if (!did) { HIP_TRY(hipStreamSynchronize(c.stream)); return PIXO_OK; }
    const size_t pixels = static_cast<size_t>(options->width) * options->height;
    if (!indices_out || indices_capacity < pixels) return too_small(pixels);
    HIP_TRY(hipMemcpyAsync(indices_out, c.q_index.p, pixels, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    palette_out_of(layout, palette_out, palette_len, trns_len, trns);
    return PIXO_OK;
}

int pixo_hip_png_quantize_device(const void *d_pixels, const pixo_png_options *options, const pixo_png_quantization *quantization, void *d_indices,
                                 uint8_t (*palette_out)[4], uint32_t *palette_len, uint32_t *trns_len, uint8_t *applied)
{
    int rc = png_check_options(options);
    if (rc) return rc;
    PIXO_REQUIRE(d_pixels);
    if ((rc = png_check_quantization(quantization))) return rc;
    PIXO_REQUIRE(d_indices);
    PIXO_REQUIRE(palette_out);
    PIXO_REQUIRE(palette_len);
    PIXO_REQUIRE(trns_len);
    PIXO_REQUIRE(applied);
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    bool did = false;
    pixo_png_layout layout;
    uint32_t trns = 0;
    if ((rc = png_quantize_on_device(*c, d_pixels, *options, *quantization, &did, &layout, &trns))) return rc;
    *applied = did ? 1 : 0;
    if (did) {
        HIP_TRY(hipMemcpyAsync(d_indices, c->q_index.p, static_cast<size_t>(options->width) * options->height, hipMemcpyDeviceToDevice, c->stream));
        palette_out_of(layout, palette_out, palette_len, trns_len, trns);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PIXO_OK;
}

int pixo_hip_debug_png_dither_stats(uint64_t *chained_launches, uint64_t *band_by_band_calls, uint64_t *gave_up)
{
    if (chained_launches) *chained_launches = g_dither_chained.load(std::memory_order_relaxed);
    if (band_by_band_calls) *band_by_band_calls = g_dither_banded.load(std::memory_order_relaxed);
    if (gave_up) *gave_up = g_dither_gave_up.load(std::memory_order_relaxed);
    return PIXO_OK;
}

int pixo_hip_png_median_cut(const uint32_t *colors, const uint32_t *counts, uint32_t n, uint32_t max_colors, uint8_t (*palette_out)[4],
                            uint32_t *palette_len)
{
    PIXO_REQUIRE(colors);
    PIXO_REQUIRE(counts);
    PIXO_REQUIRE(palette_out);
    PIXO_REQUIRE(palette_len);
    if (n == 0 || n > kMaxHistColors) return fail(PIXO_ERR_COMPRESSION, "Compression error: median cut takes 1 to 8192 colours");
    std::vector<ColorCount> cs(n);
    for (uint32_t i = 0; i < n; ++i) cs[i] = {colors[i], counts[i]};
    const std::vector<uint32_t> palette = median_cut(cs, std::min<uint32_t>(max_colors, kMaxPalette));
    for (size_t i = 0; i < palette.size(); ++i)
        for (int ch = 0; ch < 4; ++ch) palette_out[i][ch] = static_cast<uint8_t>(chan(palette[i], ch));
    *palette_len = static_cast<uint32_t>(palette.size());
    return PIXO_OK;
}

} // extern "C"
