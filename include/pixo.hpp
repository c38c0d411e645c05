// pixo.hpp — C++17 host-side mirror of the reference's Rust API for the JPEG path, header-only
// over the C ABI of pixo_hip.h.  (The reference is a Rust crate and there is no Rust toolchain
// in the build image; the host side above the C ABI is therefore written in C++ with the same
// names, argument meaning and error behaviour, so that code and tests read like the
// reference's.  The Rust binding a pixo maintainer would add is shown in INTEGRATION.md and
// sketched under rust/.)
//
//   reference (leerob/pixo v0.4.1)                      here
//   pixo::ColorType                    src/color.rs:9   pixo::ColorType
//   pixo::Error / pixo::Result<T>      src/error.rs:6   pixo::Error (exception), values returned
//   pixo::jpeg::Subsampling            jpeg/mod.rs:96   pixo::jpeg::Subsampling
//   pixo::jpeg::JpegOptions + presets  jpeg/mod.rs:121  pixo::jpeg::JpegOptions
//   pixo::jpeg::JpegOptionsBuilder     jpeg/mod.rs:230  pixo::jpeg::JpegOptionsBuilder
//   pixo::jpeg::encode                 jpeg/mod.rs:88   pixo::jpeg::encode
//   pixo::jpeg::encode_into            jpeg/mod.rs:328  pixo::jpeg::encode_into
//   (wasm) encode_jpeg                 wasm.rs:113      pixo::encode_jpeg
//   pixo::resize::ResizeAlgorithm      resize.rs:33     pixo::resize::ResizeAlgorithm
//   pixo::resize::ResizeOptions + builder resize.rs:65  pixo::resize::ResizeOptions / ResizeOptionsBuilder
//   pixo::resize::resize / resize_into resize.rs:165    pixo::resize::resize / resize_into
//   (wasm) resizeImage                 wasm.rs:183      pixo::resize_image
//   (a loop over pixo::resize::resize)                  pixo::resize::resize_batch / resize_batch_device
//   (a loop over pixo::decode::decode_png)              pixo::decode::decode_png_batch
//   (a loop over pixo::png::encode, one size each)      pixo::png::encode_images
//   (a loop over pixo::jpeg::encode, one size each)     pixo::jpeg::encode_images / encode_images_device
//   (bin) to_grayscale / rgba_to_rgb / gray_alpha_to_gray  bin/pixo.rs:478  pixo::convert::convert / convert_images / convert_images_device
#pragma once
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "pixo_hip.h"

namespace pixo {

enum class ColorType : uint8_t { Gray = 0, GrayAlpha = 1, Rgb = 2, Rgba = 3 };

constexpr size_t bytes_per_pixel(ColorType c)
{
    return c == ColorType::Gray ? 1 : c == ColorType::GrayAlpha ? 2 : c == ColorType::Rgb ? 3 : 4;
}

// pixo::Error: one kind per variant this path can raise; what() is the reference's Display text.
class Error : public std::runtime_error {
  public:
    enum class Kind {
        InvalidDimensions, InvalidDataLength, InvalidQuality, ImageTooLarge, UnsupportedColorType,
        CompressionError, InvalidRestartInterval, InvalidColorArgument, BufferTooSmall, InvalidDecode, UnsupportedDecode, Unknown
    };
    Error(Kind k, const std::string &msg) : std::runtime_error(msg), kind_(k) {}
    Kind kind() const { return kind_; }
    static Error from_status(int status)
    {
        Kind k = Kind::Unknown;
        switch (status) {
        case PIXO_ERR_INVALID_DIMENSIONS: k = Kind::InvalidDimensions; break;
        case PIXO_ERR_INVALID_DATA_LENGTH: k = Kind::InvalidDataLength; break;
        case PIXO_ERR_INVALID_QUALITY: k = Kind::InvalidQuality; break;
        case PIXO_ERR_IMAGE_TOO_LARGE: k = Kind::ImageTooLarge; break;
        case PIXO_ERR_UNSUPPORTED_COLOR_TYPE: k = Kind::UnsupportedColorType; break;
        case PIXO_ERR_COMPRESSION: k = Kind::CompressionError; break;
        case PIXO_ERR_INVALID_RESTART_INTERVAL: k = Kind::InvalidRestartInterval; break;
        case PIXO_ERR_INVALID_COLOR_ARG: k = Kind::InvalidColorArgument; break;
        case PIXO_ERR_BUFFER_TOO_SMALL: k = Kind::BufferTooSmall; break;
        case PIXO_ERR_INVALID_DECODE: k = Kind::InvalidDecode; break;
        case PIXO_ERR_UNSUPPORTED_DECODE: k = Kind::UnsupportedDecode; break;
        default: break;
        }
        return Error(k, pixo_hip_last_error());
    }

  private:
    Kind kind_;
};

namespace jpeg {

enum class Subsampling : uint8_t { S444 = 0, S420 = 1 };

class JpegOptionsBuilder;

// jpeg/mod.rs:121-157; Default = quality 75, 4:4:4, RGB, no restarts, width/height 0.
struct JpegOptions {
    uint32_t width = 0;
    uint32_t height = 0;
    ColorType color_type = ColorType::Rgb;
    uint8_t quality = 75;
    Subsampling subsampling = Subsampling::S444;
    std::optional<uint16_t> restart_interval;
    bool optimize_huffman = false;
    bool progressive = false;
    bool trellis_quant = false;

    static JpegOptions fast(uint32_t w, uint32_t h, uint8_t q) { return from_preset(w, h, q, 0); }
    static JpegOptions balanced(uint32_t w, uint32_t h, uint8_t q) { return from_preset(w, h, q, 1); }
    static JpegOptions max(uint32_t w, uint32_t h, uint8_t q) { return from_preset(w, h, q, 2); }
    static JpegOptions from_preset(uint32_t w, uint32_t h, uint8_t q, uint8_t preset)
    { // jpeg/mod.rs:162-216
        pixo_jpeg_options c;
        pixo_jpeg_options_from_preset(&c, w, h, q, preset);
        JpegOptions o;
        o.width = c.width; o.height = c.height; o.quality = c.quality;
        o.color_type = static_cast<ColorType>(c.color_type);
        o.subsampling = static_cast<Subsampling>(c.subsampling);
        o.optimize_huffman = c.optimize_huffman; o.progressive = c.progressive; o.trellis_quant = c.trellis_quant;
        return o;
    }
    static JpegOptionsBuilder builder(uint32_t width, uint32_t height);

    pixo_jpeg_options to_c() const
    {
        pixo_jpeg_options c{};
        c.width = width; c.height = height;
        c.color_type = static_cast<uint8_t>(color_type); c.quality = quality;
        c.subsampling = static_cast<uint8_t>(subsampling);
        c.has_restart_interval = restart_interval.has_value();
        c.restart_interval = restart_interval.value_or(0);
        c.optimize_huffman = optimize_huffman; c.progressive = progressive; c.trellis_quant = trellis_quant;
        return c;
    }
};

// jpeg/mod.rs:230-300
class JpegOptionsBuilder {
  public:
    JpegOptionsBuilder(uint32_t width, uint32_t height) { o_.width = width; o_.height = height; }
    JpegOptionsBuilder &color_type(ColorType v) { o_.color_type = v; return *this; }
    JpegOptionsBuilder &quality(uint8_t v) { o_.quality = v; return *this; }
    JpegOptionsBuilder &subsampling(Subsampling v) { o_.subsampling = v; return *this; }
    JpegOptionsBuilder &restart_interval(std::optional<uint16_t> v) { o_.restart_interval = v; return *this; }
    JpegOptionsBuilder &optimize_huffman(bool v) { o_.optimize_huffman = v; return *this; }
    JpegOptionsBuilder &progressive(bool v) { o_.progressive = v; return *this; }
    JpegOptionsBuilder &trellis_quant(bool v) { o_.trellis_quant = v; return *this; }
    // keeps width, height, colour type and quality (jpeg/mod.rs:285-293)
    JpegOptionsBuilder &preset(uint8_t p)
    {
        const ColorType keep = o_.color_type;
        o_ = JpegOptions::from_preset(o_.width, o_.height, o_.quality, p);
        o_.color_type = keep;
        return *this;
    }
    JpegOptions build() const { return o_; }

  private:
    JpegOptions o_;
};

inline JpegOptionsBuilder JpegOptions::builder(uint32_t width, uint32_t height)
{
    return JpegOptionsBuilder(width, height);
}

// pixo::jpeg::encode_into (jpeg/mod.rs:328): clears and refills `output`; throws pixo::Error and
// leaves `output` untouched on failure (validation precedes output.clear() in the reference).
inline void encode_into(std::vector<uint8_t> &output, const uint8_t *data, size_t len, const JpegOptions &options)
{
    const pixo_jpeg_options c = options.to_c();
    uint8_t *buf = nullptr;
    size_t n = 0;
    const int rc = pixo_hip_jpeg_encode(data, len, &c, &buf, &n);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    output.assign(buf, buf + n);
    pixo_hip_free(buf);
}

// pixo::jpeg::encode (jpeg/mod.rs:88)
[[nodiscard]] inline std::vector<uint8_t> encode(const uint8_t *data, size_t len, const JpegOptions &options)
{
    std::vector<uint8_t> out;
    encode_into(out, data, len, options);
    return out;
}
[[nodiscard]] inline std::vector<uint8_t> encode(const std::vector<uint8_t> &data, const JpegOptions &options)
{
    return encode(data.data(), data.size(), options);
}

// Images of individual sizes, gray or RGB, anywhere in one block (image i at images[i].offset: the records of
// decode::decode_png_batch and resize::fit_images) -> their files, file i byte for byte what `encode` makes of image i with
// `options` at its width, height and colour type; the options' own are not read (contract: pixo_hip.h).  With baseline options
// the launches follow the classes of images present, not their number.  The host form takes the block in host memory, the
// device form (encode_images_device) a block in HBM on the current HIP device.
namespace detail {
template <class Call> std::vector<std::vector<uint8_t>> images_files(size_t count, Call &&call)
{
    const uint32_t batch = static_cast<uint32_t>(count > 0xFFFFFFFFull ? 0xFFFFFFFFull : count);
    std::vector<uint8_t *> files(batch ? batch : 1, nullptr);
    std::vector<size_t> lens(batch ? batch : 1, 0);
    const int rc = call(batch, files.data(), lens.data());
    if (rc != PIXO_OK) throw Error::from_status(rc);
    struct Blocks { // (released also when a copy below throws)
        std::vector<uint8_t *> &files;
        ~Blocks() { for (uint8_t *f : files) pixo_hip_free(f); }
    } blocks{files};
    std::vector<std::vector<uint8_t>> out(batch);
    for (uint32_t i = 0; i < batch; ++i) out[i].assign(files[i], files[i] + lens[i]);
    return out;
}
} // namespace detail
[[nodiscard]] inline std::vector<std::vector<uint8_t>> encode_images(const uint8_t *block, size_t len, const std::vector<pixo_png_image> &images,
                                                                     const JpegOptions &options)
{
    const pixo_jpeg_options c = options.to_c();
    const pixo_png_image none{}; // (no images: the batch check answers, not the null check in front of it)
    return detail::images_files(images.size(), [&](uint32_t batch, uint8_t **files, size_t *lens) {
        return pixo_hip_jpeg_encode_images(block, len, images.empty() ? &none : images.data(), batch, &c, files, lens);
    });
}
[[nodiscard]] inline std::vector<std::vector<uint8_t>> encode_images(const std::vector<uint8_t> &block, const std::vector<pixo_png_image> &images,
                                                                     const JpegOptions &options)
{
    return encode_images(block.data(), block.size(), images, options);
}
[[nodiscard]] inline std::vector<std::vector<uint8_t>> encode_images_device(const void *d_pixels, const std::vector<pixo_png_image> &images,
                                                                            const JpegOptions &options)
{
    const pixo_jpeg_options c = options.to_c();
    const pixo_png_image none{};
    return detail::images_files(images.size(), [&](uint32_t batch, uint8_t **files, size_t *lens) {
        return pixo_hip_jpeg_encode_images_device(d_pixels, images.empty() ? &none : images.data(), batch, &c, files, lens);
    });
}

} // namespace jpeg

namespace png {
// pixo::png::FilterStrategy in declaration order (src/png/mod.rs:345-364)
enum class FilterStrategy : uint8_t { None = 0, Sub, Up, Average, Paeth, MinSum, Adaptive, AdaptiveFast, Bigrams };

namespace filter {
// pixo::png::filter::apply_filters (src/png/filter.rs:51-206): one filter-type byte + the filtered row for every
// row — what the reference hands to its DEFLATE.  `adler32`, when given, receives the zlib checksum of the
// returned bytes (src/simd/fallback.rs:8-25, computed once over the whole stream: src/compress/deflate.rs:1044).
[[nodiscard]] inline std::vector<uint8_t> apply_filters(const uint8_t *data, size_t len, uint32_t width, uint32_t height,
                                                        size_t bytes_per_pixel, FilterStrategy strategy,
                                                        uint32_t *adler32 = nullptr, uint32_t flags = 0)
{
    std::vector<uint8_t> out((size_t)height * ((size_t)width * bytes_per_pixel + 1));
    uint32_t ad = 0;
    const int rc = pixo_hip_png_filter(data, len, width, height, (uint32_t)bytes_per_pixel, (uint8_t)strategy, flags,
                                       out.data(), out.size(), &ad);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    if (adler32) *adler32 = ad;
    return out;
}
} // namespace filter

// PngOptions::flags: the device DEFLATE's denser effort for the whole-file entries (pixo_hip.h, PIXO_PNG_EFFORT_HIGH)
constexpr uint32_t kEffortHigh = PIXO_PNG_EFFORT_HIGH;

// The fields of pixo::png::PngOptions (src/png/mod.rs:41-100).  compression_level selects the zlib header's FLEVEL; the
// device DEFLATE has two efforts, but neither knob of the reference selects one: optimal_compression compresses the default
// way, and the denser effort is flags = kEffortHigh.
enum class QuantizationMode : uint8_t { Off = PIXO_PNG_QUANT_OFF, Auto = PIXO_PNG_QUANT_AUTO, Force = PIXO_PNG_QUANT_FORCE };
// pixo::png::QuantizationOptions: Off, 256 colours, no dithering by default
struct QuantizationOptions {
    QuantizationMode mode = QuantizationMode::Off;
    uint16_t max_colors = 256;
    bool dithering = false;
    pixo_png_quantization to_c() const { return pixo_png_quantization{(uint8_t)mode, (uint8_t)dithering, max_colors}; }
};
struct PngOptions {
    uint32_t width = 0, height = 0;
    ColorType color_type = ColorType::Rgba;
    uint8_t compression_level = 2;
    FilterStrategy filter_strategy = FilterStrategy::AdaptiveFast;
    bool optimize_alpha = false, reduce_color_type = false, strip_metadata = false, reduce_palette = false, optimal_compression = false;
    uint32_t flags = 0; // PIXO_PNG_NO_RAYON | kEffortHigh (the latter read by the whole-file entries)
    QuantizationOptions quantization; // travels beside pixo_png_options (pixo_png_quantization)

    // mod.rs:129-198
    static PngOptions from_preset(uint32_t width, uint32_t height, uint8_t preset)
    {
        pixo_png_options c;
        pixo_hip_png_options_from_preset(&c, width, height, preset);
        PngOptions o;
        o.width = c.width; o.height = c.height;
        o.compression_level = c.compression_level;
        o.filter_strategy = static_cast<FilterStrategy>(c.filter_strategy);
        o.optimize_alpha = c.optimize_alpha; o.reduce_color_type = c.reduce_color_type; o.reduce_palette = c.reduce_palette;
        o.strip_metadata = c.strip_metadata; o.optimal_compression = c.optimal_compression;
        return o;
    }
    static PngOptions fast(uint32_t w, uint32_t h) { return from_preset(w, h, 0); }
    static PngOptions balanced(uint32_t w, uint32_t h) { return from_preset(w, h, 1); }
    static PngOptions max(uint32_t w, uint32_t h) { return from_preset(w, h, 2); }
    static PngOptions from_preset_with_lossless(uint32_t w, uint32_t h, uint8_t preset, bool lossless) // mod.rs:203-213
    {
        PngOptions o = from_preset(w, h, preset);
        if (!lossless) o.quantization = QuantizationOptions{QuantizationMode::Auto, 256, true};
        return o;
    }
    pixo_png_options to_c() const
    {
        return pixo_png_options{width, height, (uint8_t)color_type, (uint8_t)filter_strategy, optimize_alpha, reduce_color_type,
                                reduce_palette, compression_level, optimal_compression, strip_metadata, flags};
    }
};

// What `encode_into` hands to its DEFLATE (`filtered`, mod.rs:561) after maybe_reduce_color_type and
// maybe_optimize_alpha, and what it writes into IHDR / PLTE / tRNS for it (mod.rs:526-547).
struct Prepared {
    std::vector<uint8_t> stream;
    pixo_png_layout layout;
    uint32_t adler32 = 0;
};
[[nodiscard]] inline Prepared prepare(const uint8_t *data, size_t len, const PngOptions &options)
{
    Prepared p;
    p.stream.resize((size_t)options.height * ((size_t)options.width * bytes_per_pixel(options.color_type) + 1));
    const pixo_png_options c = options.to_c();
    size_t n = 0;
    const int rc = pixo_hip_png_prepare(data, len, &c, p.stream.data(), p.stream.size(), &n, &p.layout, &p.adler32);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    p.stream.resize(n);
    return p;
}

// pixo::png::encode_with_options: a finished PNG file.  The chunks around IDAT are the reference's byte for byte; the IDAT
// body is the device DEFLATE of the prepared stream (contract: pixo_hip.h).
// ... with quantisation (mod.rs:469-511): the reference's gate decides between the indexed file and the lossless one
[[nodiscard]] inline std::vector<uint8_t> encode(const uint8_t *data, size_t len, const PngOptions &options, const QuantizationOptions &quantization)
{
    const pixo_png_options c = options.to_c();
    const pixo_png_quantization q = quantization.to_c();
    uint8_t *file = nullptr;
    size_t n = 0;
    const int rc = quantization.mode == QuantizationMode::Off ? pixo_hip_png_encode(data, len, &c, &file, &n) : pixo_hip_png_encode_lossy(data, len, &c, &q, &file, &n);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    std::vector<uint8_t> out(file, file + n);
    pixo_hip_free(file);
    return out;
}
// ... with the options' own `quantization` (Off by default: the lossless file)
[[nodiscard]] inline std::vector<uint8_t> encode(const uint8_t *data, size_t len, const PngOptions &options)
{
    return encode(data, len, options, options.quantization);
}
[[nodiscard]] inline std::vector<uint8_t> encode(const std::vector<uint8_t> &data, const PngOptions &options)
{
    return encode(data.data(), data.size(), options);
}
// `batch` equally sized images back to back in `data` -> their files, each byte for byte what `encode` makes of its image:
// one pass of filters, DEFLATE and CRC over all of them (contract: pixo_hip.h).  The options' own `quantization` is passed
// on when it is not Off.
[[nodiscard]] inline std::vector<std::vector<uint8_t>> encode_batch(const uint8_t *data, size_t len, const PngOptions &options, uint32_t batch)
{
    const pixo_png_options c = options.to_c();
    const pixo_png_quantization q = options.quantization.to_c();
    std::vector<uint8_t *> files(batch ? batch : 1, nullptr);
    std::vector<size_t> lens(batch ? batch : 1, 0);
    const int rc = pixo_hip_png_encode_batch(data, len, &c, options.quantization.mode == QuantizationMode::Off ? nullptr : &q, batch, files.data(), lens.data());
    if (rc != PIXO_OK) throw Error::from_status(rc);
    struct Blocks { // (released also when a copy below throws)
        std::vector<uint8_t *> &files;
        ~Blocks() { for (uint8_t *f : files) pixo_hip_free(f); }
    } blocks{files};
    std::vector<std::vector<uint8_t>> out(batch);
    for (uint32_t i = 0; i < batch; ++i) out[i].assign(files[i], files[i] + lens[i]);
    return out;
}
[[nodiscard]] inline std::vector<std::vector<uint8_t>> encode_batch(const std::vector<uint8_t> &data, const PngOptions &options, uint32_t batch)
{
    return encode_batch(data.data(), data.size(), options, batch);
}
// Images of individual sizes and colour types anywhere in `block` (what decode::decode_png_batch works from: image i at
// images[i].offset) -> their files, file i byte for byte what `encode` makes of image i with `options` at its width, height
// and colour type; the options' own are not read (contract: pixo_hip.h).  `quantization` is passed on when it is not Off.
[[nodiscard]] inline std::vector<std::vector<uint8_t>> encode_images(const uint8_t *block, size_t len, const std::vector<pixo_png_image> &images,
                                                                     const PngOptions &options)
{
    const pixo_png_options c = options.to_c();
    const pixo_png_quantization q = options.quantization.to_c();
    const uint32_t batch = static_cast<uint32_t>(images.size() > 0xFFFFFFFFull ? 0xFFFFFFFFull : images.size());
    std::vector<uint8_t *> files(batch ? batch : 1, nullptr);
    std::vector<size_t> lens(batch ? batch : 1, 0);
    const pixo_png_image none{}; // (no images: the batch check answers, not the null check in front of it)
    const int rc = pixo_hip_png_encode_images(block, len, images.empty() ? &none : images.data(), batch, &c, options.quantization.mode == QuantizationMode::Off ? nullptr : &q,
                                              files.data(), lens.data());
    if (rc != PIXO_OK) throw Error::from_status(rc);
    struct Blocks { // (released also when a copy below throws)
        std::vector<uint8_t *> &files;
        ~Blocks() { for (uint8_t *f : files) pixo_hip_free(f); }
    } blocks{files};
    std::vector<std::vector<uint8_t>> out(batch);
    for (uint32_t i = 0; i < batch; ++i) out[i].assign(files[i], files[i] + lens[i]);
    return out;
}
} // namespace png

namespace resize {
// resize.rs:33-45; Default = Bilinear
enum class ResizeAlgorithm : uint8_t { Nearest = 0, Bilinear = 1, Lanczos3 = 2 };

class ResizeOptionsBuilder;

// resize.rs:65-79
struct ResizeOptions {
    uint32_t src_width = 0, src_height = 0;
    uint32_t dst_width = 0, dst_height = 0;
    ColorType color_type = ColorType::Rgba;
    ResizeAlgorithm algorithm = ResizeAlgorithm::Bilinear;
    static ResizeOptionsBuilder builder(uint32_t src_width, uint32_t src_height);
    pixo_resize_options c() const
    {
        pixo_resize_options o;
        o.src_width = src_width; o.src_height = src_height;
        o.dst_width = dst_width; o.dst_height = dst_height;
        o.color_type = (uint8_t)color_type; o.algorithm = (uint8_t)algorithm;
        return o;
    }
};

// resize.rs:94-150: the destination defaults to the source size, the colour type to Rgba, the algorithm to Bilinear
class ResizeOptionsBuilder {
  public:
    ResizeOptionsBuilder(uint32_t src_width, uint32_t src_height)
    {
        o_.src_width = o_.dst_width = src_width;
        o_.src_height = o_.dst_height = src_height;
    }
    ResizeOptionsBuilder &dst(uint32_t width, uint32_t height) { o_.dst_width = width; o_.dst_height = height; return *this; }
    ResizeOptionsBuilder &color_type(ColorType c) { o_.color_type = c; return *this; }
    ResizeOptionsBuilder &algorithm(ResizeAlgorithm a) { o_.algorithm = a; return *this; }
    [[nodiscard]] ResizeOptions build() const { return o_; }

  private:
    ResizeOptions o_;
};
inline ResizeOptionsBuilder ResizeOptions::builder(uint32_t src_width, uint32_t src_height) { return ResizeOptionsBuilder(src_width, src_height); }

// pixo::resize::resize_into (resize.rs:182): `output` is cleared and resized to the result
inline void resize_into(std::vector<uint8_t> &output, const uint8_t *data, size_t len, const ResizeOptions &options)
{
    const pixo_resize_options c = options.c();
    size_t n = 0;
    output.clear();
    int rc = pixo_hip_resize_into(output.data(), 0, data, len, &c, &n); // (the checks, and the length needed)
    if (rc == PIXO_ERR_BUFFER_TOO_SMALL) {
        output.resize(n);
        rc = pixo_hip_resize_into(output.data(), output.size(), data, len, &c, &n);
    }
    if (rc != PIXO_OK) throw Error::from_status(rc);
}
// pixo::resize::resize (resize.rs:165)
[[nodiscard]] inline std::vector<uint8_t> resize(const uint8_t *data, size_t len, const ResizeOptions &options)
{
    std::vector<uint8_t> out;
    resize_into(out, data, len, options);
    return out;
}
[[nodiscard]] inline std::vector<uint8_t> resize(const std::vector<uint8_t> &data, const ResizeOptions &options)
{
    return resize(data.data(), data.size(), options);
}
// device pixels -> device pixels, enqueued on `stream` (a hipStream_t)
inline void resize_device(const void *d_src, const ResizeOptions &options, void *d_dst, void *stream = nullptr)
{
    const pixo_resize_options c = options.c();
    const int rc = pixo_hip_resize_device(d_src, &c, d_dst, stream);
    if (rc != PIXO_OK) throw Error::from_status(rc);
}
// Batches: N sources of individual sizes -> N images of one size, back to back (contract: pixo_hip.h).  Device pixels,
// enqueued on `stream`: image i lands at d_dst + i * dst_width * dst_height * bytes_per_pixel(color_type)
inline void resize_batch_device(const std::vector<pixo_resize_source> &sources, uint32_t dst_width, uint32_t dst_height, ColorType color_type,
                                ResizeAlgorithm algorithm, void *d_dst, void *stream = nullptr)
{
    const int rc = pixo_hip_resize_batch_device(sources.data(), (uint32_t)sources.size(), dst_width, dst_height, (uint8_t)color_type,
                                                (uint8_t)algorithm, d_dst, stream);
    if (rc != PIXO_OK) throw Error::from_status(rc);
}
// ... host pixels -> the images in one vector, image after image
[[nodiscard]] inline std::vector<uint8_t> resize_batch(const std::vector<pixo_resize_source> &sources, uint32_t dst_width, uint32_t dst_height,
                                                       ColorType color_type, ResizeAlgorithm algorithm)
{
    uint8_t *block = nullptr;
    size_t n = 0;
    const int rc = pixo_hip_resize_batch(sources.data(), (uint32_t)sources.size(), dst_width, dst_height, (uint8_t)color_type, (uint8_t)algorithm,
                                         &block, &n);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    struct Block { // (released also when the copy below throws)
        uint8_t *p;
        ~Block() { pixo_hip_free(p); }
    } held{block};
    return std::vector<uint8_t>(block, block + n);
}
// Images of individual sizes and colour types anywhere in one block, described by pixo_png_image records as a decode batch
// fills them in (contract: pixo_hip.h).  The sizes alone, on the host: every source at the largest size of its proportions
// inside box_width x box_height, laid out with 16-byte starts; *total: the end of the last image
[[nodiscard]] inline std::vector<pixo_png_image> fit_images(const std::vector<pixo_png_image> &src_images, uint32_t box_width, uint32_t box_height,
                                                            bool no_enlarge = false, size_t *total = nullptr)
{
    std::vector<pixo_png_image> fitted(src_images.size());
    size_t end = 0;
    const int rc = pixo_hip_resize_images_fit(src_images.data(), (uint32_t)src_images.size(), box_width, box_height,
                                              no_enlarge ? PIXO_RESIZE_FIT_NO_ENLARGE : 0u, fitted.data(), &end);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    if (total) *total = end;
    return fitted;
}
// Device pixels, enqueued on `stream`: image i at d_src + src_images[i].offset -> dst_images[i]'s size at d_dst + its offset
inline void resize_images_device(const void *d_src, const std::vector<pixo_png_image> &src_images, void *d_dst,
                                 const std::vector<pixo_png_image> &dst_images, ResizeAlgorithm algorithm, void *stream = nullptr)
{
    if (src_images.size() != dst_images.size()) throw std::invalid_argument("resize_images_device: as many destinations as sources");
    const int rc = pixo_hip_resize_images_device(d_src, src_images.data(), d_dst, dst_images.data(), (uint32_t)src_images.size(), (uint8_t)algorithm, stream);
    if (rc != PIXO_OK) throw Error::from_status(rc);
}
// ... a block in host memory -> one block laid out as dst_images says
[[nodiscard]] inline std::vector<uint8_t> resize_images(const uint8_t *data, size_t len, const std::vector<pixo_png_image> &src_images,
                                                        const std::vector<pixo_png_image> &dst_images, ResizeAlgorithm algorithm)
{
    if (src_images.size() != dst_images.size()) throw std::invalid_argument("resize_images: as many destinations as sources");
    uint8_t *block = nullptr;
    size_t n = 0;
    const int rc = pixo_hip_resize_images(data, len, src_images.data(), dst_images.data(), (uint32_t)src_images.size(), (uint8_t)algorithm, &block, &n);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    struct Block { // (released also when the copy below throws)
        uint8_t *p;
        ~Block() { pixo_hip_free(p); }
    } held{block};
    return std::vector<uint8_t>(block, block + n);
}
} // namespace resize

// Colour conversion between a decode and an encode (contract: pixo_hip.h): drop the alpha channel in front of a JPEG, or go
// gray, for one image or for N images of individual sizes and colour types in one pass.
namespace convert {
enum class Target : uint8_t { Opaque = PIXO_CONVERT_OPAQUE, Gray = PIXO_CONVERT_GRAY };
namespace detail {
inline std::vector<uint8_t> take_block(uint8_t *block, size_t n)
{
    struct Block { // (released also when the copy below throws)
        uint8_t *p;
        ~Block() { pixo_hip_free(p); }
    } held{block};
    return std::vector<uint8_t>(block, block + n);
}
} // namespace detail
// The sizes alone, on the host: every source at its own size in the colour type `target` gives it, laid out with 16-byte
// starts; *total: the end of the last image
[[nodiscard]] inline std::vector<pixo_png_image> layout_images(const std::vector<pixo_png_image> &src_images, Target target, size_t *total = nullptr)
{
    std::vector<pixo_png_image> laid(src_images.size());
    size_t end = 0;
    const int rc = pixo_hip_convert_images_layout(src_images.data(), (uint32_t)src_images.size(), (uint8_t)target, laid.data(), &end);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    if (total) *total = end;
    return laid;
}
// Device pixels, enqueued on `stream`: image i at d_src + src_images[i].offset -> dst_images[i]'s colour type at d_dst + its offset
inline void convert_images_device(const void *d_src, const std::vector<pixo_png_image> &src_images, void *d_dst,
                                  const std::vector<pixo_png_image> &dst_images, void *stream = nullptr)
{
    if (src_images.size() != dst_images.size()) throw std::invalid_argument("convert_images_device: as many destinations as sources");
    const int rc = pixo_hip_convert_images_device(d_src, src_images.data(), d_dst, dst_images.data(), (uint32_t)src_images.size(), stream);
    if (rc != PIXO_OK) throw Error::from_status(rc);
}
// ... a block in host memory -> one block laid out as dst_images says
[[nodiscard]] inline std::vector<uint8_t> convert_images(const uint8_t *data, size_t len, const std::vector<pixo_png_image> &src_images,
                                                         const std::vector<pixo_png_image> &dst_images)
{
    if (src_images.size() != dst_images.size()) throw std::invalid_argument("convert_images: as many destinations as sources");
    uint8_t *block = nullptr;
    size_t n = 0;
    const int rc = pixo_hip_convert_images(data, len, src_images.data(), dst_images.data(), (uint32_t)src_images.size(), &block, &n);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    return detail::take_block(block, n);
}
// One image: device pixels, enqueued on `stream` ...
inline void convert_device(const void *d_src, uint32_t width, uint32_t height, ColorType src, ColorType dst, void *d_dst, void *stream = nullptr)
{
    const int rc = pixo_hip_convert_device(d_src, width, height, (uint8_t)src, (uint8_t)dst, d_dst, stream);
    if (rc != PIXO_OK) throw Error::from_status(rc);
}
// ... host pixels -> the converted pixels
[[nodiscard]] inline std::vector<uint8_t> convert(const uint8_t *data, size_t len, uint32_t width, uint32_t height, ColorType src, ColorType dst)
{
    uint8_t *block = nullptr;
    size_t n = 0;
    const int rc = pixo_hip_convert(data, len, width, height, (uint8_t)src, (uint8_t)dst, &block, &n);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    return detail::take_block(block, n);
}
} // namespace convert

namespace decode {
// decode/png.rs:18-28
struct PngImage {
    uint32_t width = 0;
    uint32_t height = 0;
    std::vector<uint8_t> pixels;
    ColorType color_type = ColorType::Rgb;
};
// pixo::decode::decode_png (decode/png.rs:101)
[[nodiscard]] inline PngImage decode_png(const uint8_t *data, size_t len)
{
    uint8_t *buf = nullptr;
    size_t n = 0;
    PngImage im;
    uint8_t ct = 0;
    const int rc = pixo_hip_png_decode(data, len, &buf, &n, &im.width, &im.height, &ct);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    im.pixels.assign(buf, buf + n);
    pixo_hip_free(buf);
    im.color_type = static_cast<ColorType>(ct);
    return im;
}
[[nodiscard]] inline PngImage decode_png(const std::vector<uint8_t> &data) { return decode_png(data.data(), data.size()); }
// Batches: N files -> N images, image i what decode_png makes of file i (contract: pixo_hip.h).  one_thread: the inflates
// run on the calling thread instead of the library's small pool.  device_inflate (opt-in): the inflates run on the device, one
// wavefront per stream (PIXO_DECODE_DEVICE_INFLATE); the host inflates again only what the device does not vouch for
[[nodiscard]] inline std::vector<PngImage> decode_png_batch(const std::vector<pixo_png_file> &files, bool one_thread = false,
                                                            bool device_inflate = false)
{
    uint8_t *block = nullptr;
    size_t n = 0;
    std::vector<pixo_png_image> images(files.size() ? files.size() : 1);
    const uint32_t flags = (one_thread ? PIXO_DECODE_ONE_THREAD : 0u) | (device_inflate ? PIXO_DECODE_DEVICE_INFLATE : 0u);
    const int rc = pixo_hip_png_decode_batch(files.data(), (uint32_t)files.size(), flags, &block, &n, images.data());
    if (rc != PIXO_OK) throw Error::from_status(rc);
    struct Block { // (released also when a copy below throws)
        uint8_t *p;
        ~Block() { pixo_hip_free(p); }
    } held{block};
    std::vector<PngImage> out(files.size());
    for (size_t i = 0; i < files.size(); ++i) {
        const pixo_png_image &im = images[i];
        out[i].width = im.width; out[i].height = im.height; out[i].color_type = static_cast<ColorType>(im.color_type);
        out[i].pixels.assign(block + im.offset, block + im.offset + (size_t)im.width * im.height * (im.color_type + 1u));
    }
    return out;
}

// decode/jpeg.rs:22-31
struct JpegImage {
    uint32_t width = 0;
    uint32_t height = 0;
    std::vector<uint8_t> pixels;
    ColorType color_type = ColorType::Rgb;
};
// pixo::decode::decode_jpeg (decode/jpeg.rs:738): a baseline file -> Gray or Rgb pixels, byte for byte libjpeg-turbo's
// defaults (contract, refusals and the departures from the reference's decoder: pixo_hip.h)
[[nodiscard]] inline JpegImage decode_jpeg(const uint8_t *data, size_t len)
{
    uint8_t *buf = nullptr;
    size_t n = 0;
    JpegImage im;
    uint8_t ct = 0;
    const int rc = pixo_hip_jpeg_decode(data, len, &buf, &n, &im.width, &im.height, &ct);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    im.pixels.assign(buf, buf + n);
    pixo_hip_free(buf);
    im.color_type = static_cast<ColorType>(ct);
    return im;
}
[[nodiscard]] inline JpegImage decode_jpeg(const std::vector<uint8_t> &data) { return decode_jpeg(data.data(), data.size()); }
// Batches: N files -> N images, image i what decode_jpeg makes of file i.  one_thread: the entropy decodes run on the calling
// thread instead of the library's small pool.  device_entropy (opt-in): the Huffman decode runs on the device; the host decodes
// again only what the device does not vouch for, and the images and refusals are the same (PIXO_DECODE_DEVICE_ENTROPY).
[[nodiscard]] inline std::vector<JpegImage> decode_jpeg_batch(const std::vector<pixo_png_file> &files, bool one_thread = false, bool device_entropy = false)
{
    uint8_t *block = nullptr;
    size_t n = 0;
    std::vector<pixo_png_image> images(files.size() ? files.size() : 1);
    const uint32_t flags = (one_thread ? PIXO_DECODE_ONE_THREAD : 0u) | (device_entropy ? PIXO_DECODE_DEVICE_ENTROPY : 0u);
    const int rc = pixo_hip_jpeg_decode_batch(files.data(), (uint32_t)files.size(), flags, &block, &n, images.data());
    if (rc != PIXO_OK) throw Error::from_status(rc);
    struct Block { // (released also when a copy below throws)
        uint8_t *p;
        ~Block() { pixo_hip_free(p); }
    } held{block};
    std::vector<JpegImage> out(files.size());
    for (size_t i = 0; i < files.size(); ++i) {
        const pixo_png_image &im = images[i];
        out[i].width = im.width; out[i].height = im.height; out[i].color_type = static_cast<ColorType>(im.color_type);
        out[i].pixels.assign(block + im.offset, block + im.offset + (size_t)im.width * im.height * (im.color_type + 1u));
    }
    return out;
}
// ... into caller storage on the device (enqueue only on `stream`): image i at d_pixels + the returned records' offset, the
// records what resize::fit_images, resize::resize_images_device and jpeg::encode_images_device take unchanged.
inline std::vector<pixo_png_image> decode_jpeg_batch_device(const std::vector<pixo_png_file> &files, void *d_pixels, size_t capacity,
                                                            void *stream = nullptr, bool one_thread = false, bool device_entropy = false)
{
    std::vector<pixo_png_image> images(files.size() ? files.size() : 1);
    const uint32_t flags = (one_thread ? PIXO_DECODE_ONE_THREAD : 0u) | (device_entropy ? PIXO_DECODE_DEVICE_ENTROPY : 0u);
    const int rc = pixo_hip_jpeg_decode_batch_device(files.data(), (uint32_t)files.size(), flags, d_pixels, capacity, images.data(), stream);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    images.resize(files.size());
    return images;
}
} // namespace decode

// The reference's flat wasm export `resizeImage` (src/wasm.rs:183-201), same seven arguments.
[[nodiscard]] inline std::vector<uint8_t> resize_image(const uint8_t *data, size_t len, uint32_t src_width, uint32_t src_height,
                                                       uint32_t dst_width, uint32_t dst_height, uint8_t color_type, uint8_t algorithm)
{
    uint8_t *buf = nullptr;
    size_t n = 0;
    const int rc = pixo_hip_resize_image(data, len, src_width, src_height, dst_width, dst_height, color_type, algorithm, &buf, &n);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    std::vector<uint8_t> out(buf, buf + n);
    pixo_hip_free(buf);
    return out;
}

// The reference's flat wasm export (src/wasm.rs:113-142), same seven arguments.
[[nodiscard]] inline std::vector<uint8_t> encode_jpeg(const uint8_t *data, size_t len, uint32_t width, uint32_t height,
                                                      uint8_t color_type, uint8_t quality, uint8_t preset,
                                                      bool subsampling_420)
{
    uint8_t *buf = nullptr;
    size_t n = 0;
    const int rc = pixo_hip_encode_jpeg(data, len, width, height, color_type, quality, preset, subsampling_420, &buf, &n);
    if (rc != PIXO_OK) throw Error::from_status(rc);
    std::vector<uint8_t> out(buf, buf + n);
    pixo_hip_free(buf);
    return out;
}

} // namespace pixo
