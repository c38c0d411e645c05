// png_reduce_api.cpp — the extern "C" PNG prepare entry points: the reference's pixel reductions (png_reduce.hip) in front
// of the row filters, and the palette ordering that runs on the host (src/png/mod.rs:513-568, :683-1120).
#include "capi_internal.hpp"
#include "png_filter.hpp"
#include "png_reduce.hpp"

#include <algorithm>
#include <vector>

using namespace pixo_capi;
using namespace pixo_pngr;

namespace {
constexpr uint32_t kPngMaxDimension = 1u << 24; // mod.rs:21

// Everything small the reductions exchange with the host, the same layout on both sides.
struct PngWork {
    pixo_dev::PngAnalysis analysis;
    uint64_t lookup[kSetSlots]; // colour key -> index into the sorted keys
    uint8_t map[256];           // sorted-key index -> final palette index
    uint32_t hist[256];         // pixels per sorted-key index
    uint32_t pairs[256 * 256];  // [a * n + b], a < b: adjacent pixel pairs with the indices {a, b}
};

uint8_t png_color_type_byte(uint8_t ct) { return ct == PIXO_GRAY ? 0 : ct == PIXO_GRAY_ALPHA ? 4 : ct == PIXO_RGB ? 2 : 6; }

// optimize_palette_order's three steps on the statistics instead of the index image.  order[k] = sorted-key index of
// final entry k.  Counters are u32 and wrap like the reference's release build; delta is isize (64 bits on the hosts this
// library runs on).
void palette_order(const uint32_t *counts, const uint32_t *matrix, uint32_t n, std::vector<uint32_t> &order)
{
    order.resize(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    if (n <= 2) return; // mod.rs:916
    auto m = [&](uint32_t a, uint32_t b) { return matrix[static_cast<size_t>(a) * n + b]; };

    // weighted_edges (:980-991): (j, i) for j < i in row order, stable sort by weight descending
    struct Edge { uint32_t a, b, w; };
    std::vector<Edge> edges;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < i; ++j)
            if (m(i, j) > 0) edges.push_back({j, i, m(i, j)});
    if (edges.empty()) return; // :925
    std::stable_sort(edges.begin(), edges.end(), [](const Edge &x, const Edge &y) { return x.w > y.w; });

    // mzeng_reindex (:998-1059)
    std::vector<uint32_t> remap{edges[0].a, edges[0].b};
    struct Sum { uint32_t index, sum; };
    std::vector<Sum> sums;
    size_t best_pos = 0;
    Sum best{0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        if (i == remap[0] || i == remap[1]) continue;
        const uint32_t sum = m(i, remap[0]) + m(i, remap[1]);
        if (sum > best.sum) { best_pos = sums.size(); best = {i, sum}; }
        sums.push_back({i, sum});
    }
    while (!sums.empty()) {
        const uint32_t best_index = best.index;
        const int64_t placed = static_cast<int64_t>(n) - static_cast<int64_t>(sums.size());
        int64_t delta = 0;
        for (size_t i = 0; i < remap.size(); ++i) delta += (placed - 1 - 2 * static_cast<int64_t>(i)) * static_cast<int64_t>(m(best_index, remap[i]));
        if (delta > 0) remap.insert(remap.begin(), best_index);
        else remap.push_back(best_index);
        sums[best_pos] = sums.back(); // swap_remove
        sums.pop_back();
        best_pos = 0;
        best = {0, 0};
        for (size_t i = 0; i < sums.size(); ++i) {
            sums[i].sum += m(best_index, sums[i].index);
            if (sums[i].sum > best.sum) { best_pos = i; best = sums[i]; }
        }
    }

    // apply_most_popular_first (:1063-1099): max_by_key keeps the LAST maximum
    uint32_t len = 0;
    for (uint32_t i = 0; i < n; ++i) len += counts[i];
    uint32_t popular = remap[0], popular_count = counts[remap[0]];
    for (uint32_t idx : remap)
        if (counts[idx] >= popular_count) { popular = idx; popular_count = counts[idx]; }
    if (popular_count >= len * 3u / 20u) {
        const size_t pos = static_cast<size_t>(std::find(remap.begin(), remap.end(), popular) - remap.begin());
        if (pos >= remap.size() / 2) {
            std::reverse(remap.begin(), remap.end());
            std::rotate(remap.begin(), remap.end() - static_cast<long>(pos + 1), remap.end()); // rotate_right(pos + 1)
        } else {
            std::rotate(remap.begin(), remap.begin() + static_cast<long>(pos), remap.end()); // rotate_left(pos)
        }
    }
    order = remap;
}

// The palette case: index image, statistics, order on the host, packed rows.  an: the analysis on the host.
int reduce_to_palette(Context &c, const void *d_px, const pixo_png_options &o, PngWork *host, PngWork *dev, pixo_png_layout *layout,
                      ConvertArgs *conv)
{
    std::vector<uint32_t> keys;
    for (uint32_t s = 0; s < kSetSlots; ++s)
        if (host->analysis.table[s] & kSlotUsed) keys.push_back(static_cast<uint32_t>(host->analysis.table[s]));
    std::sort(keys.begin(), keys.end());
    const uint32_t n = static_cast<uint32_t>(keys.size());
    if (n == 0 || n > 256 || n != host->analysis.count) return fail(PIXO_ERR_COMPRESSION, "Compression error: colour set of the PNG analysis is inconsistent");
    std::fill(host->lookup, host->lookup + kSetSlots, uint64_t{0});
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t s = key_hash(keys[i]);
        while (host->lookup[s] & kSlotUsed) s = (s + 1) & (kSetSlots - 1);
        host->lookup[s] = kSlotUsed | (static_cast<uint64_t>(i) << 32) | keys[i];
    }
    const uint64_t pixels = static_cast<uint64_t>(o.width) * o.height;
    if (const int rc = reserve16(c.q_index, pixels)) return rc;
    HIP_TRY(hipMemcpyAsync(dev->lookup, host->lookup, sizeof(host->lookup), hipMemcpyHostToDevice, c.stream));
    HIP_TRY(pixo_dev::launch_png_index(d_px, pixels, bytes_per_pixel(o.color_type), dev->lookup, c.q_index.as<uint8_t>(), dev->hist, c.stream));
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    if (n > 2) {
        HIP_TRY(pixo_dev::launch_png_cooccurrence(c.q_index.as<uint8_t>(), o.width, o.height, n, dev->pairs, c.stream));
        HIP_TRY(hipMemcpyAsync(host->hist, dev->hist, sizeof(host->hist) + static_cast<size_t>(n) * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        std::vector<uint32_t> matrix(static_cast<size_t>(n) * n, 0);
        for (uint32_t a = 0; a < n; ++a)
            for (uint32_t b = a + 1; b < n; ++b) matrix[a * n + b] = matrix[b * n + a] = host->pairs[a * n + b];
        palette_order(host->hist, matrix.data(), n, order);
    }
    layout->color_type_byte = 3;
    layout->bit_depth = static_cast<uint8_t>(palette_bits(n));
    layout->bytes_per_pixel = 1;
    layout->palette_len = n;
    layout->has_trns = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t key = keys[order[k]];
        host->map[order[k]] = static_cast<uint8_t>(k);
        layout->palette[k][0] = static_cast<uint8_t>(key >> 24);
        layout->palette[k][1] = static_cast<uint8_t>(key >> 16);
        layout->palette[k][2] = static_cast<uint8_t>(key >> 8);
        layout->palette[k][3] = static_cast<uint8_t>(key);
        if ((key & 0xFFu) != 255) layout->has_trns = 1;
    }
    HIP_TRY(hipMemcpyAsync(dev->map, host->map, sizeof(host->map), hipMemcpyHostToDevice, c.stream));
    conv->form = FORM_INDEX;
    conv->spp = 1;
    conv->bits = layout->bit_depth;
    return PIXO_OK;
}

} // namespace

int pixo_capi::png_check_image(uint32_t width, uint32_t height, uint8_t color_type)
{
    if (width == 0 || height == 0) return bad_dimensions(width, height);
    if (width > kPngMaxDimension || height > kPngMaxDimension) return too_large(width, height, kPngMaxDimension);
    if (color_type > PIXO_RGBA) return fail(PIXO_ERR_UNSUPPORTED_COLOR_TYPE, "Unsupported color type for this format");
    return PIXO_OK;
}

int pixo_capi::png_check_options(const pixo_png_options *o, bool with_data, size_t data_len, uint32_t images)
{
    PIXO_REQUIRE(o);
    if (const int rc = png_check_image(o->width, o->height, o->color_type)) return rc;
    const size_t one = static_cast<size_t>(o->width) * o->height * bytes_per_pixel(o->color_type);
    const size_t want = images <= 1 || one <= SIZE_MAX / images ? one * images : SIZE_MAX; // (a batch whose bytes do not fit size_t: no length is right)
    if (with_data && data_len != want) return bad_length(want, data_len);
    if (o->filter_strategy > PIXO_PNG_BIGRAMS) return fail(PIXO_ERR_COMPRESSION, "Compression error: unknown PNG filter strategy");
    return PIXO_OK;
}

int pixo_capi::png_prepare_on_device(Context &c, const void *d_px, const pixo_png_options &o, void *d_out, pixo_png_layout *layout,
                                     size_t *out_len, uint32_t *adler, PngFilterView *view)
{
    const uint8_t ct = o.color_type;
    const uint32_t spp = bytes_per_pixel(ct);
    const uint64_t pixels = static_cast<uint64_t>(o.width) * o.height;
    std::memset(layout, 0, sizeof(*layout));
    layout->color_type_byte = png_color_type_byte(ct);
    layout->bit_depth = 8;
    layout->bytes_per_pixel = static_cast<uint8_t>(spp);

    const bool colour = ct == PIXO_RGB || ct == PIXO_RGBA, alpha = ct == PIXO_RGBA || ct == PIXO_GRAY_ALPHA;
    uint32_t want = 0;
    if (colour && o.reduce_palette) want |= pixo_dev::PNG_A_OVERFLOW; // gray inputs never build a palette (mod.rs:844-847)
    if (colour && o.reduce_color_type) want |= pixo_dev::PNG_A_NON_GRAY | (ct == PIXO_RGBA ? pixo_dev::PNG_A_NON_OPAQUE : 0u);
    if (alpha && o.optimize_alpha) want |= pixo_dev::PNG_A_ALPHA0;

    ConvertArgs conv{};
    bool convert = false;
    const void *conv_src = d_px;
    PngWork *host = nullptr, *dev = nullptr;
    if (want) {
        int rc;
        if ((rc = c.q_work.reserve(sizeof(PngWork))) || (rc = c.h_qwork.reserve(sizeof(PngWork)))) return rc;
        host = c.h_qwork.as<PngWork>();
        dev = c.q_work.as<PngWork>();
        HIP_TRY(pixo_dev::launch_png_analyse(d_px, pixels, spp, want, &dev->analysis, c.stream));
        HIP_TRY(hipMemcpyAsync(&host->analysis, &dev->analysis, sizeof(host->analysis), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        // A question the pass was asked and did not answer with "yes" was answered by reading every pixel.
        const uint32_t flags = host->analysis.flags;
        const bool zero_alpha = (want & flags & pixo_dev::PNG_A_ALPHA0) != 0; // optimize_alpha has something to do
        if ((want & pixo_dev::PNG_A_OVERFLOW) && !(flags & pixo_dev::PNG_A_OVERFLOW)) {
            // a palette image is never alpha-optimised (effective type Rgb, mod.rs:714)
            if ((rc = reduce_to_palette(c, d_px, o, host, dev, layout, &conv))) return rc;
            convert = true;
            conv_src = c.q_index.p;
        } else if (colour && o.reduce_color_type) {
            const bool gray = !(flags & pixo_dev::PNG_A_NON_GRAY), opaque = ct == PIXO_RGB || !(flags & pixo_dev::PNG_A_NON_OPAQUE);
            if (gray && opaque) { // mod.rs:736-755, :769-788
                conv.form = FORM_GRAY;
                conv.bits = gray_bits(host->analysis.gray_max);
                layout->color_type_byte = 0;
                layout->bit_depth = static_cast<uint8_t>(conv.bits);
                layout->bytes_per_pixel = 1;
                convert = true;
            } else if (ct == PIXO_RGBA && opaque) { // :789-801
                conv.form = FORM_RGB;
                layout->color_type_byte = 2;
                layout->bytes_per_pixel = 3;
                convert = true;
            } else if (ct == PIXO_RGBA && gray) { // :802-815, then optimize_alpha on GrayAlpha
                conv.form = FORM_GA;
                conv.zero_alpha = zero_alpha;
                layout->color_type_byte = 4;
                layout->bytes_per_pixel = 2;
                convert = true;
            } else if (zero_alpha) {
                conv.form = FORM_ZERO_ALPHA;
                convert = true;
            }
        } else if (zero_alpha) {
            conv.form = FORM_ZERO_ALPHA;
            convert = true;
        }
        if (conv.form != FORM_INDEX) conv.spp = spp;
    }
    layout->row_bytes = layout->bit_depth < 8 ? static_cast<uint32_t>((static_cast<uint64_t>(o.width) * layout->bit_depth + 7) / 8)
                                              : o.width * layout->bytes_per_pixel;
    *out_len = static_cast<size_t>(o.height) * (static_cast<size_t>(layout->row_bytes) + 1);

    // The filters see packed and palette rows as row_bytes one-byte pixels; the small-image rule counts PIXELS (filter.rs:77).
    const bool bytewise = layout->bit_depth < 8 || layout->color_type_byte == 3;
    const uint32_t f_width = bytewise ? layout->row_bytes : o.width, f_bpp = bytewise ? 1u : layout->bytes_per_pixel;
    if (view) *view = {f_bpp, layout->row_bytes + 1};
    int run = 0;
    bool seq = false;
    int rc = png_plan(f_width, o.height, pixels, f_bpp, o.filter_strategy, o.flags, &run, &seq);
    if (rc) return rc;
    const void *rows = d_px;
    if (convert) {
        conv.width = o.width;
        conv.height = o.height;
        conv.row_bytes = layout->row_bytes;
        if ((rc = reserve16(c.q_rows, static_cast<size_t>(layout->row_bytes) * o.height))) return rc;
        HIP_TRY(pixo_dev::launch_png_convert(conv, conv_src, dev->map, c.q_rows.p, c.stream));
        rows = c.q_rows.p;
    }
    return png_filter_on_device(c, rows, f_width, o.height, f_bpp, run, seq, d_out, adler);
}

extern "C" {

void pixo_hip_png_options_from_preset(pixo_png_options *out, uint32_t width, uint32_t height, uint8_t preset)
{
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->width = width;
    out->height = height;
    out->color_type = PIXO_RGBA;
    const bool fast = preset == 0, max = preset == 2;
    out->compression_level = fast ? 2 : max ? 9 : 6;
    out->filter_strategy = fast ? PIXO_PNG_ADAPTIVE_FAST : max ? PIXO_PNG_BIGRAMS : PIXO_PNG_ADAPTIVE;
    out->optimize_alpha = out->reduce_color_type = out->reduce_palette = out->strip_metadata = fast ? 0 : 1;
    out->optimal_compression = max ? 1 : 0;
}

int pixo_hip_png_prepare(const uint8_t *data, size_t data_len, const pixo_png_options *options, uint8_t *out, size_t out_capacity,
                         size_t *out_len, pixo_png_layout *layout, uint32_t *adler32)
{
    CallerStorageScope storage(out && out_capacity);
    int rc = png_check_options(options, true, data_len);
    if (rc) return rc;
    PIXO_REQUIRE(data);
    PIXO_REQUIRE(out_len);
    PIXO_REQUIRE(layout);
    PIXO_REQUIRE(adler32);
    const size_t full = static_cast<size_t>(options->height) * (static_cast<size_t>(options->width) * bytes_per_pixel(options->color_type) + 1);
    PIXO_THREAD_CONTEXT(c);
    if ((rc = upload(c, c.p_in, data, data_len)) || (rc = c.p_out.reserve(full))) return rc;
    if ((rc = png_prepare_on_device(c, c.p_in.p, *options, c.p_out.p, layout, out_len, adler32))) return rc;
    if (!out || out_capacity < *out_len) return too_small(*out_len);
    HIP_TRY(hipMemcpy(out, c.p_out.p, *out_len, hipMemcpyDeviceToHost));
    return PIXO_OK;
}

int pixo_hip_png_prepare_device(const void *d_pixels, const pixo_png_options *options, void *d_out, pixo_png_layout *layout,
                                size_t *out_len, uint32_t *adler32)
{
    int rc = png_check_options(options);
    if (rc) return rc;
    PIXO_REQUIRE(d_pixels);
    PIXO_REQUIRE(d_out);
    PIXO_REQUIRE(layout);
    PIXO_REQUIRE(out_len);
    PIXO_REQUIRE(adler32);
    Context *c = nullptr;
    if ((rc = context_on_current_device(&c))) return rc;
    return png_prepare_on_device(*c, d_pixels, *options, d_out, layout, out_len, adler32);
}

int pixo_hip_png_palette_order(const uint32_t *counts, const uint32_t *matrix, uint32_t n, uint8_t *order_out)
{
    PIXO_REQUIRE(counts);
    PIXO_REQUIRE(matrix);
    PIXO_REQUIRE(order_out);
    if (n == 0 || n > 256) return fail(PIXO_ERR_COMPRESSION, "Compression error: a palette has 1 to 256 entries");
    std::vector<uint32_t> order;
    palette_order(counts, matrix, n, order);
    for (uint32_t k = 0; k < n; ++k) order_out[k] = static_cast<uint8_t>(order[k]);
    return PIXO_OK;
}

} // extern "C"
