/*
 * pixo_hip.h — C ABI of the MI355X (gfx950) backend for pixo's JPEG encode path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * A Rust `pixo` crate binds these with `extern "C"` and keeps
 * its public `pixo::jpeg::{encode, encode_into, JpegOptions, …}` surface unchanged.
 * Each entry point cites the reference interface (leerob/pixo v0.4.1) it replaces.
 *
 * Threading: every function is re-entrant; device buffers and the HIP stream live
 * in a thread-local context, so many host threads may encode concurrently (the
 * reference's functions are `Sync`-safe and have rayon callers).
 *
 * Errors: functions return PIXO_OK (0) or a negative pixo_status.  The message of
 * the last failure on the calling thread — identical to the reference's
 * `pixo::Error` Display string (src/error.rs:50-91) — is available from
 * pixo_hip_last_error().  All validation errors are reported before any work is
 * done and in the reference's order (src/jpeg/mod.rs:333-373).
 */
#ifndef PIXO_HIP_H
#define PIXO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* pixo::ColorType discriminants (src/color.rs:7-18, #[repr(u8)]). */
enum { PIXO_GRAY = 0, PIXO_GRAY_ALPHA = 1, PIXO_RGB = 2, PIXO_RGBA = 3 };
/* pixo::jpeg::Subsampling (src/jpeg/mod.rs:96-101). */
enum { PIXO_S444 = 0, PIXO_S420 = 1 };

/* One code per pixo::Error variant that this path can raise (src/error.rs:10-48). */
typedef enum {
    PIXO_OK = 0,
    PIXO_ERR_INVALID_DIMENSIONS = -1,      /* Error::InvalidDimensions            */
    PIXO_ERR_INVALID_DATA_LENGTH = -2,     /* Error::InvalidDataLength            */
    PIXO_ERR_INVALID_QUALITY = -3,         /* Error::InvalidQuality               */
    PIXO_ERR_IMAGE_TOO_LARGE = -4,         /* Error::ImageTooLarge                */
    PIXO_ERR_UNSUPPORTED_COLOR_TYPE = -5,  /* Error::UnsupportedColorType         */
    PIXO_ERR_COMPRESSION = -6,             /* Error::CompressionError(String): device/runtime failures */
    PIXO_ERR_INVALID_RESTART_INTERVAL = -7,/* Error::InvalidRestartInterval       */
    PIXO_ERR_INVALID_COLOR_ARG = -8,       /* wasm.rs:122-131 "Invalid color type for JPEG: …" */
    PIXO_ERR_BUFFER_TOO_SMALL = -9,        /* encode_into with a fixed-capacity buffer */
    PIXO_ERR_INVALID_DECODE = -10,         /* Error::InvalidDecode(String): "Decode error: {msg}" (src/error.rs:83-85) */
    PIXO_ERR_UNSUPPORTED_DECODE = -11      /* Error::UnsupportedDecode(String): "Unsupported: {msg}" (src/error.rs:86-88) */
} pixo_status;

/* pixo::jpeg::JpegOptions (src/jpeg/mod.rs:121-140), field for field. */
typedef struct pixo_jpeg_options {
    uint32_t width;
    uint32_t height;
    uint8_t color_type;            /* PIXO_GRAY or PIXO_RGB                        */
    uint8_t quality;               /* 1..=100                                      */
    uint8_t subsampling;           /* PIXO_S444 / PIXO_S420                        */
    uint8_t has_restart_interval;  /* Option<u16> discriminant                     */
    uint16_t restart_interval;     /* MCUs; Some(0) is InvalidRestartInterval      */
    uint8_t optimize_huffman;
    uint8_t progressive;           /* SOF2 + simple_progressive_script (7 scans)   */
    uint8_t trellis_quant;         /* acts only with progressive, as upstream      */
} pixo_jpeg_options;

/* JpegOptions::{fast,balanced,max,from_preset} (src/jpeg/mod.rs:162-216). */
void pixo_jpeg_options_from_preset(pixo_jpeg_options *out, uint32_t width, uint32_t height,
                                   uint8_t quality, uint8_t preset);

/* ---- whole-file encode (host pixels in, JFIF bytes out) ------------------------- */

/* Replaces `pixo::jpeg::encode(data, &options) -> Result<Vec<u8>>` (src/jpeg/mod.rs:88).
 * On success *out is a block the caller releases with pixo_hip_free only (never free). */
int pixo_hip_jpeg_encode(const uint8_t *data, size_t data_len, const pixo_jpeg_options *options,
                         uint8_t **out, size_t *out_len);

/* Replaces `pixo::jpeg::encode_into(&mut output, data, &options)` (src/jpeg/mod.rs:328):
 * writes into caller storage of `capacity` bytes; *out_len receives the bytes needed
 * (also on PIXO_ERR_BUFFER_TOO_SMALL, so a Rust Vec can reserve and retry). */
int pixo_hip_jpeg_encode_into(uint8_t *output, size_t capacity, const uint8_t *data,
                              size_t data_len, const pixo_jpeg_options *options,
                              size_t *out_len);

/* Replaces the flat wasm-bindgen export `encode_jpeg(data,width,height,color_type,
 * quality,preset,subsampling_420)` (src/wasm.rs:113-142): same 7 arguments, same
 * builder order (.quality → .preset → .subsampling), same error strings. */
int pixo_hip_encode_jpeg(const uint8_t *data, size_t data_len, uint32_t width, uint32_t height,
                         uint8_t color_type, uint8_t quality, uint8_t preset,
                         int subsampling_420, uint8_t **out, size_t *out_len);

/* ---- the device seam: the coefficient tuple ------------------------------------- */

/* Geometry of `YCbCrCoefficients` (src/jpeg/mod.rs:58-61, filled by
 * compute_all_coefficients :932-1230): natural-order i16[64] blocks; 4:2:0 stores
 * Y as 4 blocks per MCU (TL,TR,BL,BR) in raster MCU order. */
int pixo_hip_coeff_geometry(uint32_t width, uint32_t height, uint8_t color_type,
                            uint8_t subsampling, size_t *y_blocks, size_t *c_blocks);

/* Fused colour → (2x2 box) → level shift → f32 AAN DCT → quantise on the GPU;
 * replaces the per-MCU loop bodies of encode_scan / compute_all_coefficients
 * (src/jpeg/mod.rs:1448-1557, :981-1046: extract_block/extract_mcu_420 + dct_2d +
 * quantize_block).  Host pointers; H2D/D2H copies included; synchronous. */
int pixo_hip_jpeg_coeffs(const uint8_t *pixels, uint32_t width, uint32_t height,
                         uint8_t color_type, uint8_t subsampling, uint8_t quality,
                         int16_t *y, size_t y_blocks, int16_t *cb, int16_t *cr,
                         size_t c_blocks);

/* Same computation on DEVICE pointers for `batch` equally-sized images laid out
 * back to back (pixels: batch*w*h*bpp bytes; y: batch*y_blocks*64 i16; …).
 * Asynchronous on `stream` (a hipStream_t, NULL = default stream). */
int pixo_hip_jpeg_coeffs_device(const void *d_pixels, uint32_t width, uint32_t height,
                                uint8_t color_type, uint8_t subsampling, uint8_t quality,
                                uint32_t batch, void *d_y, void *d_cb, void *d_cr,
                                void *stream);

/* The INTEGER secondary mode of the coefficient stage — never the default: `pixo::jpeg::encode`
 * runs the f32 transform above, and only that path gives the reference's bytes.  This entry exposes the fixed-point
 * family the reference also carries (dead code upstream): colour by the 2^16 row formulas of rgb_to_ycbcr_row_avx2
 * (src/simd/x86_64.rs:1330-1420), dct_2d_fast / dct_2d_integer (src/jpeg/dct.rs:535-568, :61-186: 13-bit fixed point,
 * per-product truncation, constant-block shortcut), quantize_block_integer (src/jpeg/dct.rs:570-583) with the
 * `*_table_int` tables (src/jpeg/quantize.rs:56-78), per 8x8 block with extract_block's edge replication
 * (src/jpeg/mod.rs:1565-1606).  4:4:4 RGB or gray (subsampling PIXO_S420 is refused); same tuple layout as above.
 * Host pointers, synchronous / device pointers of the current device, asynchronous on `stream`. */
int pixo_hip_jpeg_coeffs_integer(const uint8_t *pixels, uint32_t width, uint32_t height, uint8_t color_type,
                                 uint8_t subsampling, uint8_t quality, int16_t *y, size_t y_blocks, int16_t *cb,
                                 int16_t *cr, size_t c_blocks);
int pixo_hip_jpeg_coeffs_integer_device(const void *d_pixels, uint32_t width, uint32_t height, uint8_t color_type,
                                        uint8_t subsampling, uint8_t quality, void *d_y, void *d_cb, void *d_cr,
                                        void *stream);

/* Entropy stage on the host from a coefficient tuple (zig-zag, DC delta, run-length,
 * Huffman, byte stuffing, headers): replaces encode_block + BitWriterMsb + write_*
 * (src/jpeg/huffman.rs:423-481, src/bits.rs:195-293, src/jpeg/mod.rs:449-648) when
 * the coefficients were produced elsewhere (e.g. by several GPUs, see bands below). */
int pixo_hip_jpeg_entropy_encode(const int16_t *y, const int16_t *cb, const int16_t *cr,
                                 const pixo_jpeg_options *options, uint8_t **out,
                                 size_t *out_len);

/* Entropy stage on the DEVICE from a coefficient tuple that is already in HBM (as produced by
 * pixo_hip_jpeg_coeffs_device for ONE image): per-block Huffman coding, bit-offset prefix sum,
 * parallel packing and 0xFF stuffing on the GPU, byte-identical to encode_scan + encode_block +
 * BitWriterMsb (src/jpeg/mod.rs:1408-1563, src/jpeg/huffman.rs:423-481, src/bits.rs:195-293);
 * with options->optimize_huffman the count_block statistics (src/jpeg/mod.rs:826-860) are
 * gathered on the GPU as well, and restart intervals (src/jpeg/mod.rs:1423-1445) are handled as
 * byte-aligned segments with RSTn markers.  Only the finished file crosses PCIe.  Synchronous;
 * the pointers must belong to the current HIP device; work enqueued on the producer stream
 * (pixo_hip_set_producer_stream) is waited for on the device.  The tuple is coded as it is:
 * options->trellis_quant with progressive is refused (the tuple entries cannot re-quantise). */
int pixo_hip_jpeg_entropy_encode_device(const void *d_y, const void *d_cb, const void *d_cr,
                                        const pixo_jpeg_options *options, uint8_t **out,
                                        size_t *out_len);

/* pixo::jpeg::encode for pixels that are already in HBM (options->width * height * bpp bytes,
 * tightly packed): coefficient kernel + device entropy stage, result in a block the caller releases with
 * pixo_hip_free only (never free).
 * Same validation and errors as pixo_hip_jpeg_encode.  Ordered after the producer stream (see
 * pixo_hip_set_producer_stream), like every entry point below that takes device pixels. */
int pixo_hip_jpeg_encode_device(const void *d_pixels, const pixo_jpeg_options *options,
                                uint8_t **out, size_t *out_len);

/* The same into caller storage (`encode_into` for resident pixels): headers and the entropy-coded bytes
 * are written straight into `output` — with pinned (hipHostMalloc / registered) storage the device-to-host
 * copy is the only pass over the file.  *out_len receives the file size, also on
 * PIXO_ERR_BUFFER_TOO_SMALL (what `output` holds then is unspecified: a pinned `output` is written by the GPU directly,
 * up to its capacity).  A large scan (more than 786,432 blocks: 8192 x 4096 at
 * 4:2:0) is coded in pieces whose bytes travel while the next piece is coded — into `output` directly when
 * capacity >= 64 bytes per 8x8 block + 10 KB (a smaller `output` gets the file in one copy at the end; an `output` that
 * large may have been written to when a file larger still is refused with PIXO_ERR_BUFFER_TOO_SMALL). */
int pixo_hip_jpeg_encode_device_into(const void *d_pixels, const pixo_jpeg_options *options,
                                     uint8_t *output, size_t capacity, size_t *out_len);

/* pixo::jpeg::encode for `batch` equally sized images back to back in HBM (config 3: 64 x 1080p):
 * one coefficient launch and ONE pass of the device entropy stage for all of them — every image a byte-aligned
 * segment of the two single-pass entropy kernels — files[i] / lens[i] receive `batch` files, each a block the caller
 * releases with pixo_hip_free only (never free).  With optimize_huffman, progressive scans or restart markers the images are encoded one by one. */
int pixo_hip_jpeg_encode_batch_device(const void *d_pixels, const pixo_jpeg_options *options, uint32_t batch,
                                      uint8_t **files, size_t *lens);

/* The same into ONE block of caller storage: file i occupies arena[offsets[i], offsets[i] + lens[i]), the files follow
 * each other without gaps (offsets[0] = 0); every file is copied from the device straight to its final place — with
 * pinned (hipHostMalloc / registered) storage the device-to-host copy is the only pass over the bytes.  offsets and lens
 * have `batch` entries.  When the files do not fit, offsets / lens are still filled in (capacity needed =
 * offsets[batch - 1] + lens[batch - 1]) and PIXO_ERR_BUFFER_TOO_SMALL is returned; a null arena with capacity 0 is a size
 * query (nothing is copied).  Batches of 64 MB of pixels and more are coded in sub-batches whose files cross PCIe while the
 * next sub-batch's kernels run (two of the library's contexts alternate): an arena that turns out too small may then
 * hold the files of the first sub-batches.  `arena` may also be DEVICE memory (hipMalloc, on the current device): the
 * files then stay in HBM, complete with headers and EOI, for a caller that moves them on itself — pixo_amd/sharded.py
 * gathers the files of a batch that was scattered over several GPUs with RCCL ("C3 batch").
 * (A batch that is NOT coded in one pass — optimize_huffman, progressive scans, restart markers — reaches a device arena image by
 * image through host files: every image crosses PCIe twice there; a too small arena is noticed only after all images were coded.)
 * Replaces a loop over pixo::jpeg::encode_into (src/jpeg/mod.rs:328). */
int pixo_hip_jpeg_encode_batch_device_into(const void *d_pixels, const pixo_jpeg_options *options, uint32_t batch,
                                           uint8_t *arena, size_t capacity, size_t *offsets, size_t *lens);

/* ---- PNG row filters + Adler-32 ------------------------------ */

/* pixo::png::FilterStrategy in declaration order (src/png/mod.rs:345-364); every strategy runs on the
 * device. */
enum pixo_png_filter_strategy {
    PIXO_PNG_NONE = 0, PIXO_PNG_SUB = 1, PIXO_PNG_UP = 2, PIXO_PNG_AVERAGE = 3, PIXO_PNG_PAETH = 4,
    PIXO_PNG_MINSUM = 5, PIXO_PNG_ADAPTIVE = 6, PIXO_PNG_ADAPTIVE_FAST = 7, PIXO_PNG_BIGRAMS = 8
};
/* flags */
#define PIXO_PNG_NO_RAYON 1u /* semantics of a build without the `parallel` feature (wasm): AdaptiveFast is
                                 always the sequential, stateful variant (src/png/filter.rs:147-167) */
#define PIXO_PNG_EFFORT_HIGH 2u /* whole-file entries only (pixo_hip_png_encode*): the device DEFLATE's second, denser
                                   effort — hash chains and a one-step lazy parse — for smooth content such as screenshots,
                                   charts and gradients; see "PNG whole files" below.  Not a reference option. */

/* Replaces pixo::png::filter::apply_filters (src/png/filter.rs:51-206) and the Adler-32 the zlib
 * wrapper computes over its result (src/simd/fallback.rs:8-25, src/compress/deflate.rs:1044):
 * `out` receives height * (width * bytes_per_pixel + 1) bytes — filter-type byte + filtered row,
 * exactly what the reference hands to its DEFLATE — and *adler32 the checksum of those bytes.
 * Same strategy rules as the reference: images of <= 4096 pixels use Sub instead of the adaptive
 * strategies; the adaptive strategies treat rows independently when height > 32 (the rayon path
 * of the default build) and sequentially otherwise.  bytes_per_pixel in {1,2,3,4,6,8}.
 * Host pointers; synchronous. */
int pixo_hip_png_filter(const uint8_t *data, size_t data_len, uint32_t width, uint32_t height,
                        uint32_t bytes_per_pixel, uint8_t strategy, uint32_t flags, uint8_t *out,
                        size_t out_capacity, uint32_t *adler32);

/* Same on DEVICE pointers of the current HIP device (d_out: height * (row bytes + 1) bytes).
 * Synchronous: returns after the checksum has been combined.  The device pointers of this and of every PNG entry below
 * (d_data, d_pixels, d_out, d_indices) may have any alignment, and the results are the same bytes. */
int pixo_hip_png_filter_device(const void *d_data, uint32_t width, uint32_t height, uint32_t bytes_per_pixel,
                               uint8_t strategy, uint32_t flags, void *d_out, uint32_t *adler32);

/* Asynchronous form for resident pipelines: enqueues the filter kernel on `stream` (a
 * hipStream_t, NULL = default stream) and leaves the per-row checksum partials — two u64 per row:
 * byte sum, position-weighted byte sum — in d_row_sums[2 * height]; d_scratch is 16 bytes of
 * device memory.  pixo_hip_png_adler32_from_row_sums turns a HOST copy of the partials into the
 * zlib Adler-32 of the whole filtered stream. */
int pixo_hip_png_filter_async(const void *d_data, uint32_t width, uint32_t height, uint32_t bytes_per_pixel,
                              uint8_t strategy, uint32_t flags, void *d_out, void *d_row_sums,
                              void *d_scratch, void *stream);
uint32_t pixo_hip_png_adler32_from_row_sums(const uint64_t *row_sums, uint32_t width, uint32_t height,
                                            uint32_t bytes_per_pixel);

/* ---- PNG reductions + filters: the prepared stream (src/png/mod.rs:513-568) -------------- */

/* The prepared stream: the bytes `pixo::png::encode_into` hands to its DEFLATE (`filtered`, mod.rs:561) for given
 * pixels and options — after maybe_reduce_color_type (:683-836: palette of <= 256 colours in modified-Zeng order at
 * 1/2/4/8 bits, RGBA -> RGB / GrayAlpha / Gray, RGB -> Gray, gray bit depth), maybe_optimize_alpha (:633-671) and
 * apply_filters_with_row_bytes — together with the layout of the IHDR / PLTE / tRNS chunks that go around them.
 * pixo_hip_png_encode (below) compresses the stream on the device and writes the file; the prepare entries are for callers
 * that want the stream itself.  Quantisation (lossy) has entries of its own: pixo_hip_png_quantize and
 * pixo_hip_png_encode_lossy, below. */

/* The fields of pixo::png::PngOptions (mod.rs:64-100).  The prepare entries read the ones that shape the prepared stream.
 * pixo_hip_png_encode also reads compression_level: clamped to 1..9, it selects the FLEVEL bits of the zlib header as in the
 * reference.  The device compressor has TWO efforts, and the reference's knobs select neither: compression_level and
 * optimal_compression are accepted and compress the default way at every value, because that keeps every existing
 * caller's bytes; the denser effort is asked for with PIXO_PNG_EFFORT_HIGH in flags.  strip_metadata changes nothing,
 * because the files written here hold no chunk it would strip. */
typedef struct pixo_png_options {
    uint32_t width;
    uint32_t height;
    uint8_t color_type;        /* PIXO_GRAY .. PIXO_RGBA */
    uint8_t filter_strategy;   /* enum pixo_png_filter_strategy */
    uint8_t optimize_alpha;
    uint8_t reduce_color_type;
    uint8_t reduce_palette;
    uint8_t compression_level;
    uint8_t optimal_compression;
    uint8_t strip_metadata;
    uint32_t flags;            /* PIXO_PNG_NO_RAYON | PIXO_PNG_EFFORT_HIGH (the latter read by the whole-file entries only) */
} pixo_png_options;

/* PngOptions::{fast,balanced,max,from_preset} (mod.rs:129-198): 0 fast, 2 max, every other value balanced.
 * color_type is PIXO_RGBA, flags 0. */
void pixo_hip_png_options_from_preset(pixo_png_options *out, uint32_t width, uint32_t height, uint8_t preset);

/* What the reference writes around the IDAT data for the prepared stream (mod.rs:526-547). */
typedef struct pixo_png_layout {
    uint8_t color_type_byte;   /* IHDR colour type: 0 gray, 2 RGB, 3 palette, 4 gray + alpha, 6 RGBA */
    uint8_t bit_depth;         /* IHDR bit depth: 1, 2, 4 or 8 */
    uint8_t bytes_per_pixel;   /* the filters' distance to the "left" byte */
    uint8_t has_trns;          /* a tRNS chunk with all palette_len alphas follows PLTE (some alpha != 255) */
    uint32_t row_bytes;        /* bytes of a row without its filter byte; the stream has height * (row_bytes + 1) */
    uint32_t palette_len;      /* 0: no PLTE */
    uint8_t palette[256][4];   /* RGBA, final order */
} pixo_png_layout;

/* Host pixels -> prepared stream in `out`, its layout and the zlib Adler-32 of the stream.  *out_len receives the
 * stream's length, also on PIXO_ERR_BUFFER_TOO_SMALL; height * (width * bytes-per-pixel + 1) is always enough.
 * Checks in the reference's order (mod.rs:446-467): dimensions, a dimension above 2^24, data length.  With
 * optimize_alpha, reduce_color_type and reduce_palette all off this is pixo_hip_png_filter.  Synchronous. */
int pixo_hip_png_prepare(const uint8_t *data, size_t data_len, const pixo_png_options *options, uint8_t *out,
                         size_t out_capacity, size_t *out_len, pixo_png_layout *layout, uint32_t *adler32);

/* The same for pixels in HBM on the current HIP device: the stream is left in d_out, which must hold the unreduced
 * size height * (width * bytes-per-pixel + 1).  Ordered after the producer stream like every entry that takes device
 * pixels; synchronous, because what the image turns out to be (a palette? how many colours?) is decided on the host
 * from a few hundred bytes to a few hundred KB of statistics. */
int pixo_hip_png_prepare_device(const void *d_pixels, const pixo_png_options *options, void *d_out,
                                pixo_png_layout *layout, size_t *out_len, uint32_t *adler32);

/* The host part of the palette case (optimize_palette_order, mod.rs:909-1099), no GPU needed: from the histogram
 * counts[n] of the indices into the sorted colour keys and their n x n co-occurrence matrix (:940-977, row major;
 * the diagonal is never read) to the final order — order_out[k] is the sorted-key index of palette entry k. */
int pixo_hip_png_palette_order(const uint32_t *counts, const uint32_t *matrix, uint32_t n, uint8_t *order_out);

/* ---- PNG whole files: DEFLATE, CRC-32 and chunk writing on the device ------------------------ */

/* The contract differs from the JPEG side: the IDAT body is this library's own DEFLATE, not the reference's bytes.
 *   - Byte for byte the reference's: signature, IHDR, PLTE, tRNS, IEND (mod.rs:513-630), the two zlib header bytes for
 *     the compression level (deflate.rs:1642-1658), the Adler-32 trailer, the split into IDAT chunks of 256 KiB.
 *   - The IDAT chunks concatenated are a valid zlib stream that inflates to the prepared stream pixo_hip_png_prepare
 *     returns for the same options.
 *   - Deterministic: the same input gives the same bytes on every run.
 *   - The zlib stream is never larger than len + 5 * ceil(len / 65535) + 6 bytes (all blocks stored).
 * `out` blocks are released with pixo_hip_free, as those of the JPEG entries. */

/* Host bytes -> zlib stream (header, DEFLATE blocks of at most 65,535 input bytes each, Adler-32).  level: 1..9 after
 * clamping, header bits only.  hint_bpp / hint_row: two distances the match search tries at every position besides 1 and
 * its hash table's — for a filtered PNG stream the bytes per pixel and row_bytes + 1; 0 or a value beyond the data or the
 * 32 KiB window: not tried.  len == 0 gives the reference's empty stream (header, empty fixed block, Adler-32 of nothing). */
int pixo_hip_zlib_compress(const uint8_t *data, size_t len, uint8_t level, uint32_t hint_bpp, uint32_t hint_row,
                           uint8_t **out, size_t *out_len);
/* The same for bytes in HBM on the current HIP device, into d_out in HBM.  capacity must be at least the stored bound
 * above, 8 for len == 0 (PIXO_ERR_BUFFER_TOO_SMALL with *out_len = that size otherwise).  Synchronous.  d_data and d_out
 * may have any alignment, and the stream is the same bytes, those of pixo_hip_zlib_compress. */
int pixo_hip_zlib_compress_device(const void *d_data, size_t len, uint8_t level, uint32_t hint_bpp, uint32_t hint_row,
                                  void *d_out, size_t capacity, size_t *out_len);
/* The two entries above with the effort of the match search named: 0 is theirs (the latest occurrence of a 4-byte hash,
 * greedy parse), 1 the high effort PIXO_PNG_EFFORT_HIGH selects for whole files: up to `probes` earlier occurrences along a
 * hash chain, linked in sub-steps of `substep` positions, and a one-step lazy parse.  Slower (about twice the
 * time), needs 3 more bytes of device memory per input byte for the links, and writes smooth content much smaller; photographs
 * and noise change by a few percent at the most (INTEGRATION.md has the measured ranges).  The contract above (inflates to the input, deterministic, stored bound, one byte-aligned block
 * per 65,535 bytes) holds for both.  Any other effort: PIXO_ERR_INVALID_COLOR_ARG ("Invalid DEFLATE effort: ..."), before
 * any device work. */
int pixo_hip_zlib_compress_effort(const uint8_t *data, size_t len, uint8_t level, uint32_t hint_bpp, uint32_t hint_row,
                                  uint32_t effort, uint8_t **out, size_t *out_len);
int pixo_hip_zlib_compress_effort_device(const void *d_data, size_t len, uint8_t level, uint32_t hint_bpp, uint32_t hint_row,
                                         uint32_t effort, void *d_out, size_t capacity, size_t *out_len);
/* The high effort's two constants (png_deflate.hpp), for tests and models.  Either pointer may be NULL.  No GPU needed. */
void pixo_hip_png_deflate_effort_params(uint32_t *substep, uint32_t *probes);
/* pixo::png::encode_with_options: pixels in, a finished PNG file out.  Prepare, DEFLATE, compaction and CRC-32 run
 * without the stream leaving the device; only the finished file is copied out.  Checks: those of pixo_hip_png_prepare, in
 * the same order. */
int pixo_hip_png_encode(const uint8_t *data, size_t data_len, const pixo_png_options *options, uint8_t **out, size_t *out_len);
/* The same for pixels in HBM on the current HIP device (ordered after the producer stream); the file lands on the host. */
int pixo_hip_png_encode_device(const void *d_pixels, const pixo_png_options *options, uint8_t **out, size_t *out_len);

/* ---- PNG lossy mode: palette quantisation and dithering on the device ------------------------- */

/* pixo::png::QuantizationMode / QuantizationOptions (src/png/mod.rs).  The options travel in a struct of their own:
 * pixo_png_options keeps its 20 bytes. */
enum { PIXO_PNG_QUANT_OFF = 0, PIXO_PNG_QUANT_AUTO = 1, PIXO_PNG_QUANT_FORCE = 2 };
typedef struct pixo_png_quantization {
    uint8_t mode;        /* PIXO_PNG_QUANT_* */
    uint8_t dithering;   /* Floyd-Steinberg on r, g, b (alpha is not dithered) */
    uint16_t max_colors; /* min(max_colors, 256) everywhere; 0 behaves as 1 */
} pixo_png_quantization;

/* What encode_into does before it writes an indexed file (mod.rs:469-492): the gate — Off never, Force for RGB and RGBA, Auto
 * also needs max_colors < sampled colours <= 32 * max_colors (should_quantize_auto, :1708-1762) — then quantize_image
 * (:1505-1701): strided histogram, median cut, two k-means rounds, the 64^3 nearest-entry table, and one lookup per pixel or
 * Floyd-Steinberg dithering.  Index for index and entry for entry the reference's, with one stated exception: above 8,192
 * sampled colours the reference keeps the 8,192 most frequent by an unstable sort; here colours of equal count are kept by
 * ascending key (r<<24 | g<<16 | b<<8 | a).
 * *applied = 0: the gate declined and nothing else is written.  Otherwise width * height indices (8 bits each) go to
 * indices_out (PIXO_ERR_BUFFER_TOO_SMALL when indices_capacity is less), the palette's RGBA entries to palette_out,
 * their number to *palette_len, and *trns_len says how many alphas a tRNS chunk holds: up to the last one that is not 255
 * (maybe_trim_transparency, :1888-1902), 0 for none.  Checks: those of pixo_hip_png_prepare in its order, then a null
 * `quantization`.  Synchronous. */
int pixo_hip_png_quantize(const uint8_t *data, size_t data_len, const pixo_png_options *options,
                          const pixo_png_quantization *quantization, uint8_t *indices_out, size_t indices_capacity,
                          uint8_t (*palette_out)[4], uint32_t *palette_len, uint32_t *trns_len, uint8_t *applied);
/* The same for pixels in HBM on the current HIP device; the indices are left in d_indices (width * height bytes in HBM).
 * Only the sampled colour keys (at most about 0.5 MB) and the k-means sums cross to the host. */
int pixo_hip_png_quantize_device(const void *d_pixels, const pixo_png_options *options, const pixo_png_quantization *quantization,
                                 void *d_indices, uint8_t (*palette_out)[4], uint32_t *palette_len, uint32_t *trns_len,
                                 uint8_t *applied);
/* pixo::png::encode_with_options with quantisation: when the gate declines, exactly the bytes of pixo_hip_png_encode;
 * otherwise the indexed file of encode_indexed_into (:1814-1886): IHDR with bit depth 8 and colour type 3, PLTE, the trimmed
 * tRNS, the indices filtered as one-byte pixels — Adaptive, AdaptiveFast, MinSum and Bigrams become None, every other strategy
 * is kept — and the IDAT chunks of pixo_hip_png_encode's contract. */
int pixo_hip_png_encode_lossy(const uint8_t *data, size_t data_len, const pixo_png_options *options,
                              const pixo_png_quantization *quantization, uint8_t **out, size_t *out_len);
int pixo_hip_png_encode_lossy_device(const void *d_pixels, const pixo_png_options *options, const pixo_png_quantization *quantization,
                                     uint8_t **out, size_t *out_len);
/* ---- PNG batches: `batch` equally sized images, one pass of filters, DEFLATE and CRC ---------------- */

/* pixo::png::encode_with_options for `batch` equally sized images back to back in HBM on the current HIP device, one
 * pixo_png_options for all of them; `quantization` may be NULL (lossless).  File i is byte for byte what
 * pixo_hip_png_encode_device — pixo_hip_png_encode_lossy_device when `quantization` is given — returns for image i with the
 * same options: every strategy, preset, flag and colour type.  The DEFLATE, its scan, the compaction and the CRC-32 run as one
 * launch each over all images of a sub-batch (at most 64 MiB of prepared stream and 1024 chunks of 65,535 bytes, every image
 * counting at least one; at least one image), every image a segment no
 * match, window or aligned word crosses; with reductions, quantisation and the sequential AdaptiveFast off, so do the filters.
 * The reductions and the quantiser keep their own host round trips, image by image.
 * files[i] / lens[i] receive `batch` files, each a block the caller releases with pixo_hip_free; after a failure no block
 * stays allocated.  Checks, before the thread's context is touched: those of pixo_hip_png_encode_device on `options`, null
 * d_pixels, batch in 1..65535, `quantization` (when given) as pixo_hip_png_encode_lossy_device checks it, null files, null lens. */
int pixo_hip_png_encode_batch_device(const void *d_pixels, const pixo_png_options *options, const pixo_png_quantization *quantization,
                                     uint32_t batch, uint8_t **files, size_t *lens);
/* The same, the files back to back without gaps in `arena` — host memory, pageable or pinned — at offsets[i] (offsets[0] = 0),
 * lens[i] bytes each; both arrays have `batch` entries.  When the files do not fit, offsets / lens are still filled in
 * (capacity needed = offsets[batch - 1] + lens[batch - 1]) and PIXO_ERR_BUFFER_TOO_SMALL is returned; a null arena with
 * capacity 0 is a size query (nothing is copied).  A PNG's size is known only after compression: a size query, and a call
 * whose arena turns out too small, do all of the device work.  An arena that turns out too small may hold the files of the
 * first sub-batches.  An arena in device memory is refused. */
int pixo_hip_png_encode_batch_device_into(const void *d_pixels, const pixo_png_options *options, const pixo_png_quantization *quantization,
                                          uint32_t batch, uint8_t *arena, size_t capacity, size_t *offsets, size_t *lens);
/* ... and for host pixels: data_len must be batch x width x height x bytes per pixel (checked where pixo_hip_png_encode checks
 * its length, in front of the filter strategy). */
int pixo_hip_png_encode_batch(const uint8_t *data, size_t data_len, const pixo_png_options *options, const pixo_png_quantization *quantization,
                              uint32_t batch, uint8_t **files, size_t *lens);
/* Tests and tools: how the dither ran in this process so far — launches of the chained form, calls served band by band
 * (debug switch spin_budget=0, images of one band, or after a give-up), chained launches in which a band gave up waiting
 * (each also counts in pixo_hip_debug_lookback_fallbacks).  Null pointers are skipped. */
int pixo_hip_debug_png_dither_stats(uint64_t *chained_launches, uint64_t *band_by_band_calls, uint64_t *gave_up);
/* The host part of the quantiser, no GPU needed: median cut (median_cut_palette, :1301-1333, before its k-means) of n <= 8,192
 * colours (keys r<<24 | g<<16 | b<<8 | a) with their counts into at most min(max_colors, 256) entries, in box order. */
int pixo_hip_png_median_cut(const uint32_t *colors, const uint32_t *counts, uint32_t n, uint32_t max_colors,
                            uint8_t (*palette_out)[4], uint32_t *palette_len);

/* ---- resize (pixo::resize, src/resize.rs) ------------------------------------------------ */

/* pixo::resize::ResizeAlgorithm in declaration order (src/resize.rs:33-45). */
enum { PIXO_RESIZE_NEAREST = 0, PIXO_RESIZE_BILINEAR = 1, PIXO_RESIZE_LANCZOS3 = 2 };
#define PIXO_RESIZE_MAX_DIMENSION (1u << 24)

/* Mirrors `pixo::resize::ResizeOptions` (src/resize.rs:65-79).  The builder's defaults are
 * dst = src, PIXO_RGBA, PIXO_RESIZE_BILINEAR. */
typedef struct {
    uint32_t src_width, src_height;
    uint32_t dst_width, dst_height;
    uint8_t color_type; /* PIXO_GRAY .. PIXO_RGBA: 1-4 bytes per pixel */
    uint8_t algorithm;  /* PIXO_RESIZE_* */
} pixo_resize_options;

/* Replaces `pixo::resize::resize(data, &options)` (src/resize.rs:165): host pixels in, dst_width *
 * dst_height * bytes-per-pixel bytes out, byte for byte the reference's — also for Lanczos3, whose
 * two passes keep the reference's u8 intermediate and whose weights use the reference's sinf.
 * *out is released with pixo_hip_free.  Checks, in the reference's order: source size, destination
 * size (PIXO_ERR_INVALID_DIMENSIONS), a dimension above 2^24 (PIXO_ERR_IMAGE_TOO_LARGE), data length
 * (PIXO_ERR_INVALID_DATA_LENGTH). */
int pixo_hip_resize(const uint8_t *data, size_t data_len, const pixo_resize_options *options,
                    uint8_t **out, size_t *out_len);

/* Replaces `pixo::resize::resize_into(&mut output, data, &options)` (src/resize.rs:182): writes into
 * caller storage of `capacity` bytes; *out_len receives the bytes needed, also on
 * PIXO_ERR_BUFFER_TOO_SMALL. */
int pixo_hip_resize_into(uint8_t *output, size_t capacity, const uint8_t *data, size_t data_len,
                         const pixo_resize_options *options, size_t *out_len);

/* Same on DEVICE pointers of the current HIP device: d_src holds the source pixels, d_dst receives
 * the resized ones.  Asynchronous: the kernels are enqueued on `stream` (a hipStream_t, NULL =
 * default stream) behind what the caller enqueued on its producer stream
 * (pixo_hip_set_producer_stream), so with producer stream = `stream` the output can be handed
 * straight to pixo_hip_jpeg_encode_device or pixo_hip_png_filter_device.  The Lanczos3 intermediate
 * and tables live in the calling thread's context. */
int pixo_hip_resize_device(const void *d_src, const pixo_resize_options *options, void *d_dst,
                           void *stream);

/* The flat shape of the wasm export `resizeImage(data, src_width, src_height, dst_width, dst_height,
 * color_type, algorithm)` (src/wasm.rs:183-201): colour type, then algorithm are checked first
 * (PIXO_ERR_INVALID_COLOR_ARG), with the export's messages. */
int pixo_hip_resize_image(const uint8_t *data, size_t data_len, uint32_t src_width, uint32_t src_height,
                          uint32_t dst_width, uint32_t dst_height, uint8_t color_type, uint8_t algorithm,
                          uint8_t **out, size_t *out_len);

/* The Lanczos3 contribution table of one axis (precompute_contributions, src/resize.rs:419-462),
 * computed on the HOST, no GPU needed: for destination index d the taps are source indices
 * starts[d] .. starts[d] + counts[d], their normalised weights packed end to end in `weights`.
 * starts and counts have `dst` entries; `capacity` is the number of floats `weights` holds.  *total
 * receives the number of weights, also on PIXO_ERR_BUFFER_TOO_SMALL (null arrays with capacity 0: a
 * size query). */
int pixo_hip_resize_contributions(uint32_t src, uint32_t dst, uint32_t *starts, uint32_t *counts,
                                  float *weights, size_t capacity, size_t *total);

/* ---- resize batches: N sources of individual sizes -> N images of ONE size, back to back ---- */

/* One source of a batch: width * height * bytes-per-pixel bytes at `pixels`. */
typedef struct pixo_resize_source {
    const void *pixels;
    uint32_t width, height;
} pixo_resize_source; /* 16 bytes */

/* The stage in front of the batch encoders (pixo_hip_jpeg_encode_batch_device*, pixo_hip_png_encode_batch_device*), which
 * read `batch` equally sized images back to back: `sources` is a HOST array of `batch` (1..65535) entries whose `pixels` are
 * DEVICE pointers of the current HIP device; image i is written at d_dst + i * dst_width * dst_height * bytes-per-pixel with no
 * padding (image starts are not dword aligned in general), byte for byte what pixo_hip_resize_device writes for source i.  One
 * launch for nearest and bilinear, two for Lanczos3, whatever `batch` is: every image's workgroups read its own description.
 * Images of one width share a horizontal Lanczos3 table, images of one height a vertical one; tables and descriptions go to the
 * device in one copy.  Lanczos3 batches whose intermediates (source height rows of dst_width, padded to 16 bytes) exceed 256 MiB
 * run as sub-batches, one behind the other on `stream`.
 * Enqueue only, ordered like pixo_hip_resize_device (behind the producer stream's work); the one host wait is for the
 * calling thread's previous batch, whose tables are about to be replaced.  `sources` may be released when the call returns.
 * Checks, all before anything is enqueued (no GPU needed for a refusal): `sources`; batch (PIXO_ERR_COMPRESSION, "batch must be
 * 1..65535"); then for i = 0, 1, ... pixo_hip_resize's checks on (source i, destination, color_type, algorithm) — the first
 * failure returns that entry's status and its message with " (image i)" appended (a block of images beyond 2^62 bytes:
 * PIXO_ERR_COMPRESSION); then every `pixels`; then d_dst. */
int pixo_hip_resize_batch_device(const pixo_resize_source *sources, uint32_t batch, uint32_t dst_width, uint32_t dst_height,
                                 uint8_t color_type, uint8_t algorithm, void *d_dst, void *stream);

/* Same with HOST pixels: `pixels` are host pointers; *out receives one block of batch * dst_width * dst_height *
 * bytes-per-pixel bytes (*out_len), image after image, released with pixo_hip_free.  Returns when the block is complete. */
int pixo_hip_resize_batch(const pixo_resize_source *sources, uint32_t batch, uint32_t dst_width, uint32_t dst_height,
                          uint8_t color_type, uint8_t algorithm, uint8_t **out, size_t *out_len);

/* Tests: what the batch entries would decide for these sizes, computed on the HOST, no GPU needed (`pixels` is ignored; the
 * checks are the batch entries').  Sub-batch k is images sub_first[k] .. sub_first[k + 1] (sub_first has room for batch + 1
 * entries, *sub_count + 1 are written); mid_at[i] is image i's byte offset in its sub-batch's Lanczos3 intermediate; use_lds[i]
 * whether its horizontal pass stages source rows in LDS; *axis_tables how many distinct axis tables are built.  Nearest and
 * bilinear: one sub-batch, no tables. */
int pixo_hip_debug_resize_batch_plan(const pixo_resize_source *sources, uint32_t batch, uint32_t dst_width, uint32_t dst_height,
                                     uint8_t color_type, uint8_t algorithm, uint32_t *sub_first, uint32_t *sub_count,
                                     uint64_t *mid_at, uint8_t *use_lds, uint32_t *axis_tables);

/* ---- multi-GPU band sharding -------------------------------------- */

/* Splits the image into `parts` contiguous MCU-row bands; band `index` covers pixel
 * rows [*row_begin, *row_end) and owns *y_blocks / *c_blocks of the tuple starting
 * at block offsets *y_offset / *c_offset.  Concatenating the bands' coefficients in
 * index order gives exactly the single-device tuple (edge replication included). */
int pixo_hip_band(uint32_t width, uint32_t height, uint8_t color_type, uint8_t subsampling,
                  uint32_t parts, uint32_t index, uint32_t *row_begin, uint32_t *row_end,
                  size_t *y_offset, size_t *y_blocks, size_t *c_offset, size_t *c_blocks);

/* ---- one image across several GPUs: per-band entropy coding + splice ------------ */

/* The reference has no device boundary; its seam for this is the scan loop's only cross-MCU state: the
 * three DC predictors and the bit writer's position (src/jpeg/mod.rs:1417-1419, src/bits.rs:216-272).
 * A band (pixo_hip_band) is coded on its own GPU given (1) the last DCs of the band above and (2) the
 * bit offset at which it starts in the scan; what the GPUs exchange is 3 x i16 and one u64 per band
 * (plus, for optimised tables, 536 counters per band, summed) — never coefficients.  The exchange is the
 * caller's: torch.distributed all_gather between processes (pixo_amd/sharded.py), shared memory between
 * threads (pixo_hip_jpeg_encode_multi below).  Baseline scans without restart markers; other option sets
 * are refused by _create (gather the coefficient bands and use pixo_hip_jpeg_entropy_encode_device).
 * Calls on one encoder must not overlap; different encoders may run on different threads at once. */
#define PIXO_HIP_COUNT_WORDS 536 /* [class 0 luminance, 1 chrominance][12 DC categories + 256 AC run/size symbols] */
typedef struct pixo_hip_band_encoder pixo_hip_band_encoder;

/* Band `index` of `parts` of the image `options` describes, on HIP device `device`. */
int pixo_hip_band_encoder_create(const pixo_jpeg_options *options, uint32_t parts, uint32_t index, int device,
                                 pixo_hip_band_encoder **out);
void pixo_hip_band_encoder_destroy(pixo_hip_band_encoder *encoder);
/* pixel rows [*row_begin, *row_end) of the image belong to this band (equal: more bands than MCU rows) */
int pixo_hip_band_encoder_rows(const pixo_hip_band_encoder *encoder, uint32_t *row_begin, uint32_t *row_end);
/* Step 1: the coefficient kernel over the band's rows (`band_pixels`: those rows only, tightly packed; a
 * host pointer — copied over this GPU's own PCIe link — or, with on_device != 0, a pointer on the
 * encoder's device).  last_dc: quantised DC of the band's last Y, Cb, Cr block — what the NEXT band's
 * first blocks predict from (encode_block's return value, src/jpeg/huffman.rs:480).  A band without
 * rows reports zeros; its successor takes the DCs of the nearest band above that has rows. */
int pixo_hip_band_encoder_coeffs(pixo_hip_band_encoder *encoder, const void *band_pixels, int on_device,
                                 int16_t last_dc[3]);
/* Step 2, only with optimize_huffman: the band's count_block statistics (src/jpeg/mod.rs:826-860) given its
 * predecessors' DCs.  The tables are built from the element-wise SUM over all bands. */
int pixo_hip_band_encoder_count(pixo_hip_band_encoder *encoder, const int16_t prev_dc[3],
                                uint64_t counts[PIXO_HIP_COUNT_WORDS]);
/* Step 3: the band's length in bits (total_counts: the summed statistics, NULL without optimize_huffman). */
int pixo_hip_band_encoder_lengths(pixo_hip_band_encoder *encoder, const int16_t prev_dc[3],
                                  const uint64_t *total_counts, uint64_t *bits);
/* Step 4: Huffman-code, pack and 0xFF-stuff the band at `bit_offset` (the sum of the bits of all bands
 * before it) -> *piece (pixo_hip_free): 16 header bytes { head_nbits, head_bits, tail_nbits, tail_bits,
 * 0,0,0,0, body_len u64 LE } + body.  head = the band's first (8 - bit_offset % 8) % 8 bits (they share a
 * byte with the band before), body = its whole bytes, stuffed, tail = the bits left over. */
int pixo_hip_band_encoder_pack(pixo_hip_band_encoder *encoder, uint64_t bit_offset, uint8_t **piece,
                               size_t *piece_len);
/* Step 4 without the copy: the stuffed body stays in the encoder's device buffer (*d_body, *body_len; valid
 * until the encoder's next call; both may be NULL) and only the 16 header bytes come back.  _copy_body then
 * moves it into caller storage — typically its final place in the file (pixo_hip_jpeg_splice_layout), each
 * band over its own GPU's PCIe link; registered / pinned storage is written directly, and `dst` may also be
 * device memory (the send buffer of a collective). */
int pixo_hip_band_encoder_pack_device(pixo_hip_band_encoder *encoder, uint64_t bit_offset, uint8_t header[16],
                                      void **d_body, size_t *body_len);
int pixo_hip_band_encoder_copy_body(pixo_hip_band_encoder *encoder, uint8_t *dst);
/* Host: headers (src/jpeg/mod.rs:449-648) + the pieces of all bands in order, shared bytes merged and
 * stuffed, final 1-padding (BitWriterMsb::flush) + EOI = the file pixo::jpeg::encode writes. */
int pixo_hip_jpeg_splice(const pixo_jpeg_options *options, const uint64_t *total_counts,
                         const uint8_t *const *pieces, const size_t *piece_lens, uint32_t parts,
                         uint8_t **out, size_t *out_len);
/* The same in two steps, so that no body is copied twice: from the 16-byte headers of all pieces
 * (`piece_headers`: parts x 16 bytes) _layout tells the file's length and where every body belongs;
 * _finish writes everything else into `file` — JFIF headers, the bytes neighbouring bands share (merged and
 * stuffed), the final 1-padding, EOI. */
int pixo_hip_jpeg_splice_layout(const pixo_jpeg_options *options, const uint64_t *total_counts,
                                const uint8_t *piece_headers, uint32_t parts, size_t *file_len,
                                size_t *body_offsets);
int pixo_hip_jpeg_splice_finish(const pixo_jpeg_options *options, const uint64_t *total_counts,
                                const uint8_t *piece_headers, uint32_t parts, uint8_t *file, size_t file_len);
/* Host twins of steps 2-4 for a band whose coefficient tuple is in host memory (`band_rows` pixel rows;
 * what pixo_hip_jpeg_entropy_encode is to the whole tuple). */
int pixo_hip_jpeg_band_count_host(const int16_t *y, const int16_t *cb, const int16_t *cr,
                                  const pixo_jpeg_options *options, uint32_t band_rows, const int16_t prev_dc[3],
                                  uint64_t counts[PIXO_HIP_COUNT_WORDS]);
int pixo_hip_jpeg_band_bits_host(const int16_t *y, const int16_t *cb, const int16_t *cr,
                                 const pixo_jpeg_options *options, uint32_t band_rows, const int16_t prev_dc[3],
                                 const uint64_t *total_counts, uint64_t *bits);
int pixo_hip_jpeg_band_piece_host(const int16_t *y, const int16_t *cb, const int16_t *cr,
                                  const pixo_jpeg_options *options, uint32_t band_rows, const int16_t prev_dc[3],
                                  const uint64_t *total_counts, uint64_t bit_offset, uint8_t **piece,
                                  size_t *piece_len);

/* pixo::jpeg::encode on `n_devices` GPUs of this process (config 4: one 16384 x 16384 image over 8
 * MI355X): band k of n_devices goes to devices[k] (a device may appear more than once); every band's
 * rows are read straight from `data` over that GPU's PCIe link by its own host thread, the exchanges
 * above happen in shared memory, the calling thread splices.  Byte-identical to pixo_hip_jpeg_encode.
 * Progressive scans and restart markers are coded by devices[0] alone. */
int pixo_hip_jpeg_encode_multi(const uint8_t *data, size_t data_len, const pixo_jpeg_options *options,
                               const int *devices, uint32_t n_devices, uint8_t **out, size_t *out_len);

/* A BATCH over `n_devices` GPUs of this process (configs[2] on a node, SURVEY §8e "C3 batch"): `batch` equally sized images
 * back to back at `pixels` — memory of ANY of the process's GPUs (the images of the other GPUs' shares travel by peer copies,
 * hipMemcpyPeer: one peer per xGMI link) or host memory (every GPU fetches its share over its own PCIe link).  devices[k]
 * encodes images [batch k / n, batch (k + 1) / n) with pixo_hip_jpeg_encode_batch_device_into's one-pass kernels into its own
 * HBM, the persistent worker threads of pixo_hip_jpeg_encode_multi exchange the file lengths in shared memory, and every GPU
 * copies its run of finished files to their final place in `arena` (host memory, pinned for full speed) over its OWN PCIe
 * link.  offsets / lens / capacity / PIXO_ERR_BUFFER_TOO_SMALL as pixo_hip_jpeg_encode_batch_device_into (a null arena with
 * capacity 0 is a size query); a device may appear more than once.  Byte-identical to that entry on one GPU.
 * Device pixels: what the caller enqueued on its producer stream (pixo_hip_set_producer_stream; default the NULL stream) is waited
 * for before the workers read them — `pixels` needs no length argument, so the caller guarantees batch x image bytes behind it
 * (the Python and Rust mirrors check that).  pixo_hip_trim() also releases the workers' device buffers.
 * Replaces a loop over pixo::jpeg::encode (src/jpeg/mod.rs:88) spread over the GPUs of a node. */
int pixo_hip_jpeg_encode_batch_multi(const void *pixels, const pixo_jpeg_options *options, uint32_t batch,
                                     const int *devices, uint32_t n_devices, uint8_t *arena, size_t capacity,
                                     size_t *offsets, size_t *lens);

/* ---- PNG decode ------------------------------------------------------------------------ */

/* Replaces `pixo::decode::decode_png(data) -> Result<PngImage>` (src/decode/png.rs:101-291): a PNG file in host memory ->
 * 8-bit pixels.  The chunk walk, its checks and the inflate run on the host in the reference's order and with its messages
 * (PIXO_ERR_INVALID_DECODE / PIXO_ERR_UNSUPPORTED_DECODE, PIXO_ERR_INVALID_DIMENSIONS, PIXO_ERR_IMAGE_TOO_LARGE); row
 * reconstruction (reconstruct_image / unfilter_row, :294-410) and the conversion to pixels (convert_to_pixels, :430-533) run
 * on the device.  *color_type: the PIXO_* colour type of the pixels (:271-283: a palette image is PIXO_RGBA only if its tRNS
 * holds a value other than 255).  On success *pixels is a block of width * height * channels bytes the caller releases with
 * pixo_hip_free only. */
int pixo_hip_png_decode(const uint8_t *file, size_t len, uint8_t **pixels, size_t *pixels_len, uint32_t *width, uint32_t *height,
                        uint8_t *color_type);
/* The same walk and checks up to "no IDAT data" (src/decode/png.rs:102-260) and the colour-type rule (:271-283), nothing else:
 * no inflate, no GPU.  What a caller of pixo_hip_png_decode_device allocates from.  (What only the inflated stream can show —
 * an ill-formed stream, a filter byte above 4, a palette image without PLTE — is left to the decode.) */
int pixo_hip_png_decode_info(const uint8_t *file, size_t len, uint32_t *width, uint32_t *height, uint8_t *color_type);
/* decode_png with the pixels left in DEVICE memory: `file` is host memory, d_pixels device memory of `capacity` bytes
 * (PIXO_ERR_BUFFER_TOO_SMALL, with *width, *height and *color_type set, when that is less than width * height * channels).
 * Ordered like pixo_hip_resize_device: the upload and the kernels are enqueued on `stream` behind the work of the producer
 * stream, and the call returns without waiting for them, so the pixels can be handed on that stream to
 * pixo_hip_resize_device, pixo_hip_jpeg_encode_device or pixo_hip_png_encode_device.  Every error of pixo_hip_png_decode is
 * reported before anything is enqueued.  d_pixels may have any alignment, and the pixels are the same bytes. */
int pixo_hip_png_decode_device(const uint8_t *file, size_t len, void *d_pixels, size_t capacity, uint32_t *width, uint32_t *height,
                               uint8_t *color_type, void *stream);
/* Host only: `inflate_zlib_with_size(data, Some(expected))` (src/decode/inflate.rs:294-352) into `out` (`expected` bytes): the
 * 6-byte minimum, the three header checks, the blocks, the Adler-32 read from the LAST four bytes of `data`, then the size —
 * in that order, with the reference's messages.  Never writes past `expected` bytes. */
int pixo_hip_zlib_inflate(const uint8_t *data, size_t len, uint8_t *out, size_t expected);
/* Rows a workgroup of the reconstruction kernel walks side by side; a longer run of dependent rows takes several passes
 * (tests place their pass boundaries by it). */
uint32_t pixo_hip_png_unfilter_pass_rows(void);
/* MEASUREMENT only (tools/png_decode_timing.py): pixo_hip_png_decode with its legs timed — ms[0] chunk walk + CRC, [1] inflate,
 * [2] finding the runs of rows (host clocks), [3] upload, [4] reconstruction kernel, [5] conversion kernel (HIP events),
 * [6] the whole call; counts[0] segments (rows that do not read the row above start one), [1] rows of the longest,
 * [2] workgroups launched.  The pixels are released again. */
int pixo_hip_debug_png_decode_timed(const uint8_t *file, size_t len, double ms[7], uint64_t counts[3]);

/* ---- PNG decode batches: N files -> N images back to back in DEVICE memory, one launch per pass ---- */

/* One file of a batch, in host memory. */
typedef struct pixo_png_file {
    const uint8_t *data;
    size_t len;
} pixo_png_file; /* 16 bytes */
/* One image of the block a batch decodes into: width * height * bytes-per-pixel bytes at `offset`, of the colour type
 * pixo_hip_png_decode reports for that file (no image is converted to another's).  offset[0] = 0, offset[i + 1] = offset[i] +
 * image i's bytes rounded up to 16; the bytes between two images are never written.  `reserved` is written as zeros.  An array of
 * pixo_resize_source can point straight at d_pixels + offset. */
typedef struct pixo_png_image {
    uint64_t offset;
    uint32_t width, height;
    uint8_t color_type;
    uint8_t reserved[7];
} pixo_png_image; /* 24 bytes */
#define PIXO_DECODE_ONE_THREAD 1u /* flags bit 0: the inflates run on the calling thread (for callers that run a pool of their own) */
/* flags bit 1 (opt-in; the batch entries only): the streams are inflated ON THE DEVICE, one wavefront per stream, all streams of
 * a sub-batch in one launch (png_inflate.hip).  The compressed streams go up instead of the inflated ones; per sub-batch one
 * inflate launch, one launch that gathers the filter bytes, one small copy of status records and filter bytes down, and one
 * host wait for it.  The host then decides in index order: a stream whose device verdict is not OK, or whose Adler-32 differs
 * from the last four bytes of its IDAT data, is inflated again by the host inflate, whose result is the truth — its error is
 * returned as without the flag, its bytes replace the stream on the device.  Image i stays byte for byte what
 * pixo_hip_png_decode returns for file i.  What changes in the contract, under this flag only: phase 1 and the zlib header
 * checks (the 6-byte minimum, method, header checksum, preset dictionary) are still made before anything is enqueued, but the
 * other phase-2 refusals come AFTER the inflate launch of their sub-batch, and with several sub-batches after earlier
 * sub-batches' images were written: d_pixels is unspecified after a refusal.  The calls wait on the host once per sub-batch.
 * At most 11 launches a sub-batch.  The single-file entries never inflate on the device: one stream is one wavefront. */
#define PIXO_DECODE_DEVICE_INFLATE 2u

/* flags bit 2 (opt-in; the JPEG batch entries only, the PNG entries ignore it as the JPEG entries ignore bit 1; the single JPEG
 * entries take no flags and keep the host decoder): the Huffman decode of the scans runs ON THE DEVICE (jpeg_entropy_dec.hip).
 * Per sub-batch the raw scans and one record per file go up in one copy instead of the coefficients; a lane decodes a
 * subsequence of 128 scan bytes, exit states are handed from lane to lane until nothing changes (some launches, with a host wait
 * for a counter behind each; at most 132 rounds a file), then one launch each verifies the chains, writes the coefficients and
 * sums the DC differences, the status records come down, and the decode launches follow on coefficients that never left the
 * device.  The device VOUCHES for a file or does not; it never refuses one.  Every file it does not vouch for is decoded again
 * by the host's decoder, whose coefficients replace the device's at that file's place — or whose refusal is the call's.  The
 * host decodes from the start: files with a restart interval, files without MCUs, scans below 16 bytes and scans of 2^28 bytes
 * and more.  Image i stays byte for byte what the entry returns without the flag, and a refused batch is refused with the same
 * status and words, the failing file with the lowest index answering.  What changes in the contract, under this flag only:
 * phase 1 is still complete before anything is enqueued, but phase-2 refusals come AFTER the entropy launches of their
 * sub-batch, and with several sub-batches after earlier sub-batches' images were written: d_pixels is unspecified after a
 * refusal.  The calls wait on the host at least twice per sub-batch.  The sub-batch limit counts records and scans too. */
#define PIXO_DECODE_DEVICE_ENTROPY 4u

/* The layout alone: `images` (batch entries) and *total (the end of the last image, not rounded) from the walks of the files — no
 * inflate, no GPU.  What a caller of pixo_hip_png_decode_batch_device allocates from. */
int pixo_hip_png_decode_batch_info(const pixo_png_file *files, uint32_t batch, pixo_png_image *images, size_t *total);
/* `batch` (1..65535) files -> their pixels at d_pixels + images[i].offset, image i byte for byte what pixo_hip_png_decode returns
 * for file i.  The streams are inflated on up to 8 host threads (the caller among them, never more than files) into one pinned
 * staging buffer and go up in one copy, all tables in a second; then one reconstruction launch per distinct filter unit (at most
 * 6) and one conversion launch per kernel form (at most 3), whatever `batch` is.  Batches whose device staging (inflated streams
 * + reconstructed rows) exceeds 512 MiB run as sub-batches, one behind the other on `stream`.  Enqueue only, ordered like
 * pixo_hip_png_decode_device; the one host wait is for the calling thread's previous decode job.  d_pixels may have any alignment.
 * Checks, all before anything is enqueued.  Phase 1, no GPU and no inflate: `files`; batch (PIXO_ERR_COMPRESSION, "batch must be
 * 1..65535"); the trailing out-pointers; then for i = 0, 1, ... files[i].data and the walk of file i — the first failure returns
 * that file's status and its message with " (image i)" appended, `images` untouched; a block of pixels beyond 2^62 bytes
 * (PIXO_ERR_COMPRESSION); then `images` is filled; capacity below the total: PIXO_ERR_BUFFER_TOO_SMALL with the total in the
 * message; then d_pixels.  Phase 2, what only the inflated streams show (whatever inflate raises, Adler-32, size, a filter byte
 * above 4, a palette file without PLTE): every file is inflated, the failing file with the lowest index decides, " (image i)"
 * appended, whatever the thread count. */
int pixo_hip_png_decode_batch_device(const pixo_png_file *files, uint32_t batch, uint32_t flags, void *d_pixels, size_t capacity,
                                     pixo_png_image *images, void *stream);
/* The same with the block in HOST memory: *out receives *out_len = total bytes laid out as `images` says (the gaps hold
 * nothing of meaning), released with pixo_hip_free.  Returns when the block is complete. */
int pixo_hip_png_decode_batch(const pixo_png_file *files, uint32_t batch, uint32_t flags, uint8_t **out, size_t *out_len,
                              pixo_png_image *images);
/* Tests: what the batch entries decide, computed on the HOST (phase 1, the inflates into ordinary memory, the plan), no GPU
 * needed; refusals as the decode entries', phase 2 included.  Sub-batch k is images sub_first[k] .. sub_first[k + 1] (room for
 * batch + 1 entries, *sub_count + 1 are written); runs_per_image[i]: workgroups that reconstruct image i; the launch counts are
 * summed over the sub-batches (conversion forms as for a 16-byte aligned d_pixels); *threads: host threads that inflated. */
int pixo_hip_debug_png_decode_batch_plan(const pixo_png_file *files, uint32_t batch, uint32_t flags, uint32_t *sub_first,
                                         uint32_t *sub_count, uint64_t *runs_per_image, uint32_t *unfilter_launches,
                                         uint32_t *convert_launches, uint32_t *threads);
/* The boundaries of the device inflate (png_inflate_math.h; tests place their cases by them): tokens a step holds at most; bytes
 * of the LDS ring (DEFLATE's window); the distance beyond which a match closes its step; bytes of a stored block copied at a time. */
uint32_t pixo_hip_png_inflate_step_tokens(void);
uint32_t pixo_hip_png_inflate_window_bytes(void);
uint32_t pixo_hip_png_inflate_far_distance(void);
uint32_t pixo_hip_png_inflate_stored_chunk(void);
/* Tests and measurements: the inflate kernel alone over `n` (1..65535) zlib streams of any origin in host memory (pixo_png_file:
 * data, len >= 6; the two header bytes and the four checksum bytes are skipped, not checked).  `out` is a host block of
 * max(out_at[i] + expected[i]) bytes that the caller has filled: the whole block is uploaded, stream i is inflated on the device
 * into [out_at[i], out_at[i] + expected[i]) of it, and the block is downloaded again, so that every byte outside the regions —
 * and inside them behind produced[i] — can be checked for being untouched.  The raw device results, no host inflate behind them:
 * verdict[i] 0 OK (the final block ended at exactly expected[i] bytes), 1 FAILED, 2 NEEDS_HOST (an over-subscribed code set);
 * produced[i] bytes of region i are inflated bytes whatever the verdict, adler[i] is their Adler-32.  *kernel_ms: the inflate
 * launch's device time by HIP events. */
int pixo_hip_debug_zlib_inflate_batch_device(const pixo_png_file *streams, uint32_t n, const uint64_t *expected, uint8_t *out,
                                             const uint64_t *out_at, uint32_t *verdict, uint64_t *produced, uint32_t *adler,
                                             double *kernel_ms);
/* MEASUREMENT only (tools/png_decode_batch_timing.py): pixo_hip_png_decode_batch with its legs timed — ms[0] the inflates and
 * the runs of rows (host clock), [1] uploads, [2] reconstruction launches, [3] conversion launches (HIP events, summed over the
 * sub-batches), [4] the whole call.  The block is released again. */
int pixo_hip_debug_png_decode_batch_timed(const pixo_png_file *files, uint32_t batch, uint32_t flags, double ms[5]);

/* ---- JPEG decode: baseline files -> pixels, single and in batches (pixo::decode::decode_jpeg, src/decode/jpeg.rs:738) ----
 * The pixels are byte for byte what libjpeg-turbo produces with its defaults (islow IDCT, fancy upsampling, no smoothing): one
 * component gives PIXO_GRAY, three give PIXO_RGB.  The marker walk and the Huffman decode run on the host; dequantisation,
 * IDCT, chroma upsampling, colour conversion and the crop run on the device and leave the pixels in device memory.
 * Accepted: SOF0 with 8-bit precision; one component (its sampling factors are ignored), or three with luma 1x1, 2x1 or 2x2 and
 * both chroma 1x1 (4:4:4, 4:2:2, 4:2:0); one interleaved scan; any restart interval; up to four tables of each kind, redefined
 * between segments; DQT with 8- or 16-bit entries; APPn, COM and fill bytes in front of markers are skipped.
 * Refused, in the reference's words (PIXO_ERR_INVALID_DECODE "Decode error: ...", PIXO_ERR_UNSUPPORTED_DECODE "Unsupported:
 * ..."), in the order of its marker walk: "not a JPEG file", "unexpected end of file", "truncated marker", "invalid marker
 * length", the segments' length and table-id messages, "progressive JPEG not supported", "{n}-bit precision not supported",
 * "{n} components not supported", "no image data found".  Refused with messages of this library, at SOS behind the
 * reference's checks and in this order: no frame in front of the scan (Invalid); any other sampling, 4:4:0 included
 * (Unsupported); a scan whose components are not the frame's, in its order (Unsupported); an Adobe APP14 transform other than
 * 1 on three components (Unsupported); component ids 'R', 'G', 'B' (Unsupported); a quantisation or Huffman table the scan
 * uses and no segment defined (Invalid); a scan of less than two bits per block (Invalid); at DHT, lengths that describe no
 * prefix code (Invalid).  And from the entropy decode (Invalid): an entropy-coded segment that ends early, a code that no table
 * holds, a coefficient index past 63, a missing or out-of-sequence RSTn.
 * Two departures from the reference, on purpose.  (1) It returns a partly decoded picture when the scan breaks off; this
 * library refuses.  (2) Its three defects are not reproduced: the odd part of its IDCT is 2^-13 of its size, its bit reader
 * drops unconsumed bits at a restart marker, and its nearest-sample upsampling and 8-bit colour constants agree with no other
 * decoder.  A width or height of zero is no special case: the image has no bytes.
 * Crafted coefficients: the kernel computes in 32 bits with unsigned wrap and clamps to 0..255; libjpeg computes in long and
 * indexes a masked table.  The two agree while no intermediate leaves 32 bits and every descaled sample lies in -512..511 — no
 * encoder of 8-bit pixels leaves either; the bound on the dequantised block and its derivation: jpeg_decode_math.h. */

/* A baseline JPEG file in host memory -> *pixels (width * height * channels bytes, released with pixo_hip_free). */
int pixo_hip_jpeg_decode(const uint8_t *file, size_t len, uint8_t **pixels, size_t *pixels_len, uint32_t *width, uint32_t *height,
                         uint8_t *color_type);
/* What pixo_hip_jpeg_decode would report, from the walk up to SOS alone — no entropy decode, no GPU. */
int pixo_hip_jpeg_decode_info(const uint8_t *file, size_t len, uint32_t *width, uint32_t *height, uint8_t *color_type);
/* The same into caller storage on the device, d_pixels of `capacity` bytes at any alignment (PIXO_ERR_BUFFER_TOO_SMALL, with
 * *width, *height and *color_type set, when that is less than the image).  Enqueue only, ordered like
 * pixo_hip_png_decode_device; every refusal comes before anything is enqueued. */
int pixo_hip_jpeg_decode_device(const uint8_t *file, size_t len, void *d_pixels, size_t capacity, uint32_t *width, uint32_t *height,
                                uint8_t *color_type, void *stream);
/* The layout of a batch alone (as pixo_hip_png_decode_batch_info): the walks only — no entropy decode, no GPU. */
int pixo_hip_jpeg_decode_batch_info(const pixo_png_file *files, uint32_t batch, pixo_png_image *images, size_t *total);
/* `batch` (1..65535) files -> their pixels at d_pixels + images[i].offset, image i byte for byte what pixo_hip_jpeg_decode
 * returns for file i; offsets as in the PNG batch (multiples of 16; the bytes between two images and behind the last are never
 * written), so that pixo_hip_resize_images_fit, pixo_hip_resize_images_device, pixo_hip_convert_images_device,
 * pixo_hip_jpeg_encode_images_device and pixo_hip_png_encode_images_device take `images` unchanged.  The scans are decoded on up
 * to 8 host threads (the caller among them; PIXO_DECODE_ONE_THREAD: the caller alone) straight into pinned staging in the
 * order the kernel loads them; the records go up in one copy, a sub-batch's coefficients in a second, then one launch per class
 * present (gray, 4:4:4, 4:2:2, 4:2:0, each in a form with 16-byte stores and one with byte stores for images at odd addresses),
 * whatever `batch` is.  Batches whose coefficients exceed 512 MiB run as sub-batches, one behind the other on `stream`.
 * Enqueue only; the one host wait is for the calling thread's previous JPEG decode job.  Checks as
 * pixo_hip_png_decode_batch_device, in its order, all before anything is enqueued: phase 1 the walks (a refusal leaves `images`
 * untouched), phase 2 the entropy decodes; the failing file with the lowest index answers, " (image i)" appended, whatever the
 * thread count.  PIXO_DECODE_DEVICE_INFLATE is ignored; PIXO_DECODE_DEVICE_ENTROPY (opt-in): the Huffman decode on the device,
 * described at the flag. */
int pixo_hip_jpeg_decode_batch_device(const pixo_png_file *files, uint32_t batch, uint32_t flags, void *d_pixels, size_t capacity,
                                      pixo_png_image *images, void *stream);
/* The same with the block in HOST memory, released with pixo_hip_free. */
int pixo_hip_jpeg_decode_batch(const pixo_png_file *files, uint32_t batch, uint32_t flags, uint8_t **out, size_t *out_len,
                               pixo_png_image *images);
/* Tests: what the batch entries decide, computed on the HOST from phase 1 (no GPU): sub-batch k is images sub_first[k] ..
 * sub_first[k + 1] (room for batch + 1 entries, *sub_count + 1 are written); classes[i]: 0 gray, 1 4:4:4, 2 4:2:2, 3 4:2:0;
 * *launches summed over the sub-batches (forms as for a 16-byte aligned d_pixels); *threads: host threads that would decode. */
int pixo_hip_debug_jpeg_decode_batch_plan(const pixo_png_file *files, uint32_t batch, uint32_t flags, uint32_t *sub_first,
                                          uint32_t *sub_count, uint8_t *classes, uint32_t *launches, uint32_t *threads);
/* Tests, host only (no GPU): the quantisation tables the kernel would be handed — q[i][c][n]: image i's record, component c, natural
 * order; room for batch * 3 * 64 values.  A gray image's components 1 and 2, and an image without MCUs, are zeros. */
int pixo_hip_debug_jpeg_decode_batch_tables(const pixo_png_file *files, uint32_t batch, uint16_t *q);
/* Tests, host only: the QUANTISED coefficients of component `component` as the entropy decoder read them, 64 per block in zigzag
 * order, the blocks in raster order of the component's padded plane (*blocks_w x *blocks_h).  `capacity` counts int16 values
 * (less than blocks * 64: PIXO_ERR_BUFFER_TOO_SMALL with the two counts set). */
int pixo_hip_debug_jpeg_decode_coefficients(const uint8_t *file, size_t len, uint32_t component, int16_t *out, size_t capacity,
                                            uint32_t *blocks_w, uint32_t *blocks_h);
/* The tile of whole MCUs a workgroup of the decode kernel owns (tests place their tile boundaries by it). */
void pixo_hip_jpeg_decode_tile_mcus(uint32_t *mcus_x, uint32_t *mcus_y);
/* MEASUREMENT only (tools/jpeg_decode_batch_timing.py): pixo_hip_jpeg_decode_batch with its legs timed — ms[0] the entropy
 * decodes (host clock), [1] uploads, [2] kernels, [3] the copy of the block to the host (HIP events, summed over the
 * sub-batches), [4] the whole call.  The block is released again.  With PIXO_DECODE_DEVICE_ENTROPY [0] is the host's share
 * (building records, reading status records, decoding again what the device did not vouch for), [1] the uploads of the
 * coefficients the host decoded; the device leg: pixo_hip_debug_jpeg_entropy_last. */
int pixo_hip_debug_jpeg_decode_batch_timed(const pixo_png_file *files, uint32_t batch, uint32_t flags, double ms[5]);

/* The device Huffman decode's geometry (tests place their boundaries by it): bytes of a subsequence, subsequences a workgroup
 * owns, the round cap of a call, the shortest scan that goes to the device.  Any pointer may be null. */
void pixo_hip_jpeg_entropy_geometry(uint32_t *sub_bytes, uint32_t *group_subs, uint32_t *round_cap, uint32_t *min_scan_bytes);
/* Tests, host only (no GPU): what the batch entries decide under `flags` — on_device[i]: 1 when PIXO_DECODE_DEVICE_ENTROPY is
 * set and file i's scan would be decoded on the device, 0 when the host decodes it from the start; the sub-batches as
 * pixo_hip_debug_jpeg_decode_batch_plan reports them (which honours the flag too). */
int pixo_hip_debug_jpeg_entropy_plan(const pixo_png_file *files, uint32_t batch, uint32_t flags, uint8_t *on_device, uint32_t *sub_first,
                                     uint32_t *sub_count);
/* Tests: the device Huffman decode alone, all files in one sub-batch, no host decoder behind it.  Per file four words in
 * info: vouched (0 / 1), why not (0 vouched, 1 a dead state or a flawed lane in the chain, 2 the states had not settled at the round cap, 3 the
 * chain ends in front of the last block, 4 the host decodes this file from the start), subsequences, rounds used.  The
 * coefficients of component `component` of every vouched file that has one, in the format of
 * pixo_hip_debug_jpeg_decode_coefficients, at out + out_at[i] (int16 values; the caller sizes them by that entry); other files'
 * places are left alone.  round_cap: 0 for the library's, or a smaller one. */
int pixo_hip_debug_jpeg_entropy_batch(const pixo_png_file *files, uint32_t batch, uint32_t component, uint32_t round_cap, int16_t *out,
                                      const uint64_t *out_at, uint32_t *info);
/* MEASUREMENT (tools/jpeg_entropy_timing.py): of the calling thread's last batch call with PIXO_DECODE_DEVICE_ENTROPY — the
 * device leg in ms (HIP events from the scans' upload to the DC launch, the host waits between the launches included, summed
 * over the sub-batches), the most rounds a file used, the files sent to the device, the files the host decoded again. */
void pixo_hip_debug_jpeg_entropy_last(double *device_ms, uint32_t *rounds, uint32_t *files_device, uint32_t *files_redone);

/* ---- PNG encode of images of individual sizes and colour types, anywhere in one block ---- */

/* `batch` images anywhere in one block in HBM on the current HIP device: image i is images[i].width x images[i].height pixels
 * of images[i].color_type at d_pixels + images[i].offset (any alignment, gaps and overlaps allowed, `reserved` not read) —
 * what pixo_hip_png_decode_batch_device fills in.  `options` is a template: its width, height and color_type are NOT read;
 * `quantization` may be NULL (lossless).  File i is byte for byte what pixo_hip_png_encode_device —
 * pixo_hip_png_encode_lossy_device when `quantization` is given — returns for image i alone, called with `options` after image
 * i's width, height and colour type are written into it: every strategy, preset, flag and colour type.
 * Sub-batches as pixo_hip_png_encode_batch_device (at most 64 MiB of unreduced stream and 1024 chunks, greedy in index order,
 * at least one image); the DEFLATE, its scan, the compaction and the CRC-32 run as one launch each over all images of a
 * sub-batch.  The way in is each image's own: with quantisation, optimize_alpha, reduce_color_type and reduce_palette off
 * and the image's AdaptiveFast not the sequential form (its own height decides), its rows are filtered in a launch shared with
 * all images of its class — bytes per pixel, rows and first byte multiples of 4 or not, the filter kernel's form for its row
 * length and resolved strategy, rows that fit the LDS stage or not — so the number of filter launches follows the classes
 * present, not `batch`; every other image is prepared by itself, with its own host round trips.
 * files[i] / lens[i] receive `batch` files, each a block the caller releases with pixo_hip_free; after a failure no block
 * stays allocated.  Checks, all before the thread's context is touched, in this order: null options; an unknown
 * options->filter_strategy; null d_pixels; null images; batch in 1..65535; `quantization` (when given) as
 * pixo_hip_png_encode_lossy_device checks it; null files, null lens; then for i = 0, 1, ... image i: a zero side, a side above
 * 2^24, a colour type above 3 (statuses and messages of pixo_hip_png_encode_device's checks), offset + the image's bytes
 * beyond 2^62 (PIXO_ERR_COMPRESSION) — each with " (image i)" appended. */
int pixo_hip_png_encode_images_device(const void *d_pixels, const pixo_png_image *images, uint32_t batch, const pixo_png_options *options,
                                      const pixo_png_quantization *quantization, uint8_t **files, size_t *lens);
/* The same, the files back to back in `arena` in host memory: sink semantics and the size query exactly as
 * pixo_hip_png_encode_batch_device_into (offsets / lens filled in also with PIXO_ERR_BUFFER_TOO_SMALL; a device arena is
 * refused).  Checks as above with `offsets` in the place of `files`. */
int pixo_hip_png_encode_images_device_into(const void *d_pixels, const pixo_png_image *images, uint32_t batch, const pixo_png_options *options,
                                           const pixo_png_quantization *quantization, uint8_t *arena, size_t capacity, size_t *offsets,
                                           size_t *lens);
/* ... and for a block in host memory (what pixo_hip_png_decode_batch returns): the checks above with `data` for d_pixels, then
 * data_len below the furthest image's end: PIXO_ERR_INVALID_DATA_LENGTH, "expected <that end> bytes, got <data_len>". */
int pixo_hip_png_encode_images(const uint8_t *data, size_t data_len, const pixo_png_image *images, uint32_t batch,
                               const pixo_png_options *options, const pixo_png_quantization *quantization, uint8_t **files, size_t *lens);
/* Tests: what the entries above decide, no GPU needed.  alignment (0..15): d_pixels modulo 16.  Sub-batch k is images
 * sub_first[k] .. sub_first[k + 1] (room for batch + 1 entries, *sub_count + 1 are written); way_in[i]: 1 when image i's rows go
 * through a shared filter launch, 0 when it is prepared by itself; run_strategy[i]: the strategy png_plan resolves for the
 * unreduced image i; *filter_launches: shared filter launches summed over the sub-batches.  Checks as the entries' (no
 * pixels; alignment behind `quantization`; the five out-pointers in the place of files and lens). */
int pixo_hip_debug_png_encode_images_plan(const pixo_png_image *images, uint32_t batch, const pixo_png_options *options,
                                          const pixo_png_quantization *quantization, uint32_t alignment, uint32_t *sub_first,
                                          uint32_t *sub_count, uint8_t *way_in, uint8_t *run_strategy, uint32_t *filter_launches);

/* ---- JPEG encode of images of individual sizes and colour types, anywhere in one block ---- */

/* The JPEG end of the chain decode batch -> fit -> resize images: `batch` images anywhere in one block in HBM on the current
 * HIP device, described by the records the PNG images entries take — image i is images[i].width x images[i].height pixels of
 * images[i].color_type (PIXO_GRAY or PIXO_RGB), tightly packed, at d_pixels + images[i].offset (any alignment, gaps and
 * overlaps allowed: the pixels are only read; `reserved` is not read).  `options` is a template: its width, height and
 * color_type are NOT read; quality, subsampling, restart interval, optimize_huffman, progressive and trellis_quant hold for
 * every image.  File i is byte for byte what pixo_hip_jpeg_encode_device returns for image i alone, called with `options`
 * after image i's width, height and colour type are written into it: every preset, quality and subsampling.
 * The shared way in — no progressive scans, no optimised tables, no restart markers in the image's scan: the batch entry's
 * condition for one pass —: all images of a sub-batch go through one coefficient launch per class present (gray, or RGB at the
 * template's subsampling, times the load form: aligned rows, rows at any address, images narrower than 4 pixels), then one
 * coding pass and one stuffing pass per colour class, every image a byte-aligned segment of its own size: the number of
 * launches follows the classes present, not `batch`.  Every other image is encoded by itself in index order, and so is a
 * sub-batch whose single-pass launch gave up its bounded waits (PIXO route FALLBACK).
 * Sub-batches are greedy in index order, at least one image each, at most 2^22 blocks of 64 coefficients (512 MiB of tuple,
 * 836 MiB of packed streams; PIXO_HIP_DEBUG jpeg_images_blocks=n lowers it); a sub-batch also ends where the way changes.
 * files[i] / lens[i] receive `batch` files, each a block from the pinned pool that the caller releases with pixo_hip_free;
 * after a failure no block stays allocated.  The scans of a sub-batch reach the files in one copy per colour class through
 * the context's pinned buffer, or — when every destination is pinned and the scans total 4 MiB x max(1, images / 64) or more —
 * file by file straight into the destinations (PIXO route JPEG_IMAGES_DIRECT, bit 49, beside JPEG_IMAGES).  Checks, all before the thread's context is touched, in this order: null options;
 * the template's quality and Some(0) restart interval as pixo_hip_jpeg_encode_device checks them; null d_pixels; null images;
 * batch in 1..65535; null files, null lens; then for i = 0, 1, ... image i with the single entry's statuses and messages, each
 * with " (image i)" appended: a zero side, a side above 65535, a colour type that is not PIXO_GRAY or PIXO_RGB
 * (PIXO_ERR_UNSUPPORTED_COLOR_TYPE, also for GrayAlpha and RGBA: alpha is not dropped), then offset + the image's bytes beyond
 * 2^62 (PIXO_ERR_COMPRESSION). */
int pixo_hip_jpeg_encode_images_device(const void *d_pixels, const pixo_png_image *images, uint32_t batch, const pixo_jpeg_options *options,
                                       uint8_t **files, size_t *lens);
/* The same, the files back to back in `arena` in host memory (pinned or pageable), as pixo_hip_jpeg_encode_batch_device_into:
 * no gaps, offsets[0] = 0, offsets / lens filled in also with PIXO_ERR_BUFFER_TOO_SMALL, a null arena with capacity 0 is a
 * size query.  A device arena is refused (PIXO_ERR_COMPRESSION): the headers differ per image and are written by the host.
 * Checks as above with `offsets` in the place of `files`. */
int pixo_hip_jpeg_encode_images_device_into(const void *d_pixels, const pixo_png_image *images, uint32_t batch, const pixo_jpeg_options *options,
                                            uint8_t *arena, size_t capacity, size_t *offsets, size_t *lens);
/* ... and for a block in host memory, uploaded up to the furthest image's end: the checks above with `data` for d_pixels, then
 * data_len below that end: PIXO_ERR_INVALID_DATA_LENGTH, "expected <that end> bytes, got <data_len>". */
int pixo_hip_jpeg_encode_images(const uint8_t *data, size_t data_len, const pixo_png_image *images, uint32_t batch,
                                const pixo_jpeg_options *options, uint8_t **files, size_t *lens);
/* Tests: what the entries above decide, no GPU and no pixels needed.  alignment (0..15): d_pixels modulo 16.  Sub-batch k is
 * images sub_first[k] .. sub_first[k + 1] (room for batch + 1 entries, *sub_count + 1 are written); way_in[i]: 1 shared, 0 by
 * itself; load_form[i]: 0 aligned, 1 funnel, 2 bytes, from image i's first byte's address and its row length; first_group[i]:
 * the first group of 192 blocks of image i within its colour class's coding pass in its sub-batch (0 for the single way);
 * *coef_launches / *entropy_passes: coefficient launches / coding passes (each with its stuffing pass) summed over the
 * sub-batches.  Checks as the entries' (no pixels; alignment behind batch; the seven out-pointers in the place of files and
 * lens). */
int pixo_hip_debug_jpeg_encode_images_plan(const pixo_png_image *images, uint32_t batch, const pixo_jpeg_options *options, uint32_t alignment,
                                           uint32_t *sub_first, uint32_t *sub_count, uint8_t *way_in, uint8_t *load_form, uint64_t *first_group,
                                           uint32_t *coef_launches, uint32_t *entropy_passes);

/* ---- resize of images of individual sizes and colour types, anywhere in one block ---- */

/* The link between pixo_hip_png_decode_batch_device and pixo_hip_png_encode_images*: `batch` (1..65535) sources described by
 * src_images (what a decode batch fills in) become `batch` images described by dst_images, every one of its own size, in one
 * pass per sub-batch — decode a folder, fit it into a box, write it back, without leaving the device.
 *
 * The sizes alone, computed on the HOST, no GPU needed: dst_images[i] receives source i's colour type and the largest size of
 * source i's proportions inside box_width x box_height, as the reference's front end computes it (calculateResizeDimensions of
 * its web/src/lib/wasm.ts): in f64, aspect = sw / sh; the size is box_width x round(box_width / aspect), and where that is
 * taller than the box, round(box_height * aspect) x box_height; round is JavaScript's Math.round (a tie goes up), each side is
 * at least 1.  With PIXO_RESIZE_FIT_NO_ENLARGE in `flags`, a source that already fits the box keeps its size.  The offsets are
 * the decode batch's layout: offset[0] = 0, offset[i + 1] = offset[i] + image i's bytes rounded up to 16; *total: the end of the
 * last image, not rounded; `reserved` is written as zeros.  dst_images may be src_images.  Checks, before anything is written:
 * src_images, dst_images, total; batch (PIXO_ERR_COMPRESSION, "batch must be 1..65535"); a zero box side
 * (PIXO_ERR_INVALID_DIMENSIONS) or one above 2^24 (PIXO_ERR_IMAGE_TOO_LARGE); then for i = 0, 1, ... source i: a zero side, a
 * side above 2^24, a colour type above 3 (PIXO_ERR_INVALID_COLOR_ARG), each with " (image i)" appended; a block beyond 2^62
 * bytes (PIXO_ERR_COMPRESSION). */
#define PIXO_RESIZE_FIT_NO_ENLARGE 1u
int pixo_hip_resize_images_fit(const pixo_png_image *src_images, uint32_t batch, uint32_t box_width, uint32_t box_height,
                               uint32_t flags, pixo_png_image *dst_images, size_t *total);

/* Image i is src_images[i].width x height pixels of src_images[i].color_type at d_src + src_images[i].offset and becomes
 * dst_images[i].width x height pixels at d_dst + dst_images[i].offset — any alignment on both sides, any order — byte for byte
 * what pixo_hip_resize_device writes for (source i -> destination i, that colour type, `algorithm`).  The bytes between
 * destinations are never written.  Destinations must not overlap each other or a source: the caller's contract, NOT checked.
 * `reserved` is not read.  src_images and dst_images are HOST arrays and may be released when the call returns.
 * Every pass is a flat launch over the tiles of all images of a sub-batch, whose workgroups find their image by a binary search:
 * nearest and bilinear take one launch per bytes-per-pixel value present (at most 4); Lanczos3 one horizontal launch per
 * bytes-per-pixel value present and ONE vertical launch, whatever `batch` is.  One Lanczos3 table per distinct (source size,
 * destination size) pair per axis; tables and records go to the device in one copy.  Sub-batches, greedy in index order with at
 * least one image each, where the Lanczos3 intermediates (source height rows of the image's own destination width, padded to
 * 16 bytes) would exceed 256 MiB or a launch 2^31 - 1 tiles; they run one behind the other on `stream`.
 * Enqueue only, ordered like pixo_hip_resize_batch_device, whose buffers these entries share: behind the producer stream's
 * work, with one host wait for the calling thread's previous batch or images job, whose tables are about to be replaced.
 * Checks, all before anything is enqueued (no GPU needed for a refusal): src_images, then dst_images; batch
 * (PIXO_ERR_COMPRESSION, "batch must be 1..65535"); then for i = 0, 1, ... image i: pixo_hip_resize's checks on (source i,
 * destination i, source i's colour type, algorithm) with that entry's status and message; a colour type of destination i that
 * differs from source i's (PIXO_ERR_COMPRESSION, "Compression error: colour types differ"); offset + the image's bytes beyond
 * 2^62 on the source's, then the destination's side (PIXO_ERR_COMPRESSION) — each with " (image i)" appended, the first failing
 * image answers; then d_src, then d_dst. */
int pixo_hip_resize_images_device(const void *d_src, const pixo_png_image *src_images, void *d_dst,
                                  const pixo_png_image *dst_images, uint32_t batch, uint8_t algorithm, void *stream);

/* Same for a block in HOST memory (what pixo_hip_png_decode_batch returns): the checks above with `data` for d_src, then out,
 * out_len, then data_len below the furthest source's end: PIXO_ERR_INVALID_DATA_LENGTH, "expected <that end> bytes, got
 * <data_len>".  *out receives one block of *out_len bytes, up to the furthest destination's end, laid out as dst_images says
 * (the gaps hold nothing of meaning), released with pixo_hip_free.  Returns when the block is complete. */
int pixo_hip_resize_images(const uint8_t *data, size_t data_len, const pixo_png_image *src_images,
                           const pixo_png_image *dst_images, uint32_t batch, uint8_t algorithm, uint8_t **out, size_t *out_len);

/* Tests: what the entries above decide for these sizes, computed on the HOST, no GPU needed (offsets are checked, not used; the
 * checks are the entries' up to the images', then the out-pointers in their order).  Sub-batch k is images sub_first[k] ..
 * sub_first[k + 1] (room for batch + 1 entries, *sub_count + 1 are written); mid_at[i]: image i's byte offset in its
 * sub-batch's Lanczos3 intermediate; use_lds[i]: its horizontal pass stages source rows in LDS; tiles_first[i]: its workgroups
 * in the point pass (256 columns x 4 rows) or the horizontal pass (64 columns x 4 source rows); tiles_second[i]: in the
 * vertical pass (1024 bytes x 1 row; 0 for nearest and bilinear) — an image has at most 65535 rows of tiles a pass (debug switch
 * resize_images_rows=n: n), its workgroups stride over the rest; *axis_tables: distinct axis tables built; *launches_first /
 * *launches_second: launches of the two passes summed over the sub-batches. */
int pixo_hip_debug_resize_images_plan(const pixo_png_image *src_images, const pixo_png_image *dst_images, uint32_t batch,
                                      uint8_t algorithm, uint32_t *sub_first, uint32_t *sub_count, uint64_t *mid_at,
                                      uint8_t *use_lds, uint32_t *tiles_first, uint32_t *tiles_second, uint32_t *axis_tables,
                                      uint32_t *launches_first, uint32_t *launches_second);

/* ---- colour conversion: drop alpha or go gray, one image or N images of individual sizes, one pass ---- */

/* What the reference's front end does between a decode and an encode (src/bin/pixo.rs:478-513 gray_alpha_to_gray, rgba_to_rgb,
 * to_grayscale; :619-638 where it applies them), on pixels that stay in HBM.  The pairs (source colour type -> destination
 * colour type) that exist: equal types (a copy); GrayAlpha -> Gray (byte 0 of every pixel); Rgba -> Rgb (bytes 0..2);
 * Rgb -> Gray and Rgba -> Gray ((77 r + 150 g + 29 b + 128) >> 8, alpha ignored).  Every other pair — Gray -> Rgb, anything
 * that adds alpha — has no counterpart in the reference and is refused (PIXO_ERR_UNSUPPORTED_COLOR_TYPE, "Unsupported color
 * type for this format").  The two targets a caller names instead of a pair: */
#define PIXO_CONVERT_OPAQUE 0 /* in front of a JPEG: GrayAlpha -> Gray, Rgba -> Rgb, Gray and Rgb kept */
#define PIXO_CONVERT_GRAY 1   /* the front end's --grayscale: everything -> Gray */

/* The destinations `target` gives the sources, on the HOST only: dst_images[i] has source i's size and the colour type the
 * target gives it, laid out as a decode batch lays its block out — offset[0] = 0, every image rounded up to 16 bytes, *total the
 * end of the last image (not rounded), `reserved` zeros; the sources' offsets are not read.  dst_images may be src_images.
 * Checks, nothing is written before all have passed: src_images, dst_images, total; batch (PIXO_ERR_COMPRESSION, "batch must be
 * 1..65535"); an unknown target (PIXO_ERR_COMPRESSION, "unknown convert target"); then for i = 0, 1, ... source i: a zero side
 * (PIXO_ERR_INVALID_DIMENSIONS), a side above 2^24 (PIXO_ERR_IMAGE_TOO_LARGE), a colour type above 3
 * (PIXO_ERR_INVALID_COLOR_ARG), each with " (image i)" appended; a block beyond 2^62 bytes (PIXO_ERR_COMPRESSION). */
int pixo_hip_convert_images_layout(const pixo_png_image *src_images, uint32_t batch, uint8_t target, pixo_png_image *dst_images,
                                   size_t *total);
/* `batch` images anywhere in two blocks in HBM on the current HIP device: image i of src_images[i].width x height pixels of
 * src_images[i].color_type at d_src + src_images[i].offset -> the same pixels in dst_images[i].color_type at d_dst +
 * dst_images[i].offset, byte for byte what pixo_hip_convert_device writes for that image alone; the bytes between destinations
 * are left as they are.  Any alignment of either block and of every offset: an image whose two addresses are multiples of 16 —
 * what the decode batch's, pixo_hip_resize_images_fit's and the layout's offsets give in blocks so aligned — moves in 16-byte
 * loads and stores, any other image byte by byte.  Destinations must not overlap each other or a source (not checked).  One
 * launch per (conversion, aligned or not) present — at most 10 — whatever `batch` is; a launch holds at most 2^31 - 1
 * workgroups, batches beyond that run as sub-batches (greedy in index order, at least one image), one behind the other on
 * `stream`.  Enqueue only, ordered like pixo_hip_resize_images_device: behind the work of the producer stream; the one host
 * wait is for the calling thread's previous convert job, whose records are about to be replaced.
 * Checks, all before anything is enqueued (no GPU needed for a refusal): src_images, dst_images; batch (PIXO_ERR_COMPRESSION,
 * "batch must be 1..65535"); then for i = 0, 1, ... image i: a zero side or a side above 2^24 of the source, then of the
 * destination; a colour type above 3 of the source, then of the destination (PIXO_ERR_INVALID_COLOR_ARG); sizes that differ
 * between source i and destination i (PIXO_ERR_COMPRESSION, "Compression error: sizes differ"); a pair that is none of the
 * above (PIXO_ERR_UNSUPPORTED_COLOR_TYPE); offset + the image's bytes beyond 2^62 on the source's, then the destination's side
 * (PIXO_ERR_COMPRESSION) — each with " (image i)" appended, the first failing image answers; then d_src, d_dst. */
int pixo_hip_convert_images_device(const void *d_src, const pixo_png_image *src_images, void *d_dst, const pixo_png_image *dst_images,
                                   uint32_t batch, void *stream);
/* The same for a block in HOST memory: *out receives one block of *out_len = the furthest destination's end bytes laid out as
 * dst_images says (the gaps hold nothing of meaning), released with pixo_hip_free.  The checks above, then data, out, out_len,
 * then data_len below the furthest source's end: PIXO_ERR_INVALID_DATA_LENGTH, "expected <that end> bytes, got <data_len>". */
int pixo_hip_convert_images(const uint8_t *data, size_t data_len, const pixo_png_image *src_images, const pixo_png_image *dst_images,
                            uint32_t batch, uint8_t **out, size_t *out_len);
/* One image: width x height pixels of src_color_type at d_src -> dst_color_type at d_dst (device memory, any alignment).
 * Enqueue only, ordered like pixo_hip_resize_device.  Checks: a zero side, a side above 2^24, src_color_type then
 * dst_color_type above 3, a pair that does not exist, then d_src, d_dst. */
int pixo_hip_convert_device(const void *d_src, uint32_t width, uint32_t height, uint8_t src_color_type, uint8_t dst_color_type,
                            void *d_dst, void *stream);
/* ... host pixels in, a block released with pixo_hip_free out.  The checks above up to the pair, then out, out_len, data_len
 * other than width * height * source bytes per pixel (PIXO_ERR_INVALID_DATA_LENGTH), then data. */
int pixo_hip_convert(const uint8_t *data, size_t data_len, uint32_t width, uint32_t height, uint8_t src_color_type,
                     uint8_t dst_color_type, uint8_t **out, size_t *out_len);
/* Tests: what pixo_hip_convert_images_device decides for these records when d_src is src_align and d_dst is dst_align modulo
 * 16, computed on the HOST, no GPU needed (the entry's checks up to the images', then the out-pointers in their order).
 * Sub-batch k is images sub_first[k] .. sub_first[k + 1] (room for batch + 1 entries, *sub_count + 1 are written); kind[i]:
 * 0 copy, 1 GrayAlpha -> Gray, 2 Rgba -> Rgb, 3 Rgb -> Gray, 4 Rgba -> Gray; form[i]: 0 aligned, 1 bytes; tiles[i]: image
 * i's workgroups, one per pixo_hip_debug_convert_tile_pixels() pixels, at most 65536 (debug switch convert_images_tiles=n: n,
 * and a launch then holds at most 2n), which stride over the rest; *launches: summed over the sub-batches. */
int pixo_hip_debug_convert_images_plan(const pixo_png_image *src_images, const pixo_png_image *dst_images, uint32_t batch,
                                       uint32_t src_align, uint32_t dst_align, uint32_t *sub_first, uint32_t *sub_count,
                                       uint8_t *kind, uint8_t *form, uint32_t *tiles, uint32_t *launches);
/* Pixels of a tile, what one workgroup of the conversion kernels takes in a step (tests place their sizes by it). */
uint32_t pixo_hip_debug_convert_tile_pixels(void);

/* ---- runtime ----------------------------------------------------------------------- */

int pixo_hip_device_count(void);            /* 0 when no GPU / no driver              */
int pixo_hip_set_device(int device);        /* device for the calling thread's context (host-pointer entries) */
/* Entry points that take DEVICE pointers run on the library's own stream, ordered after everything the
 * caller has enqueued so far on `stream` (a hipStream_t of the calling thread's current device; default:
 * the NULL stream, which is also PyTorch's default stream).  Per thread. */
int pixo_hip_set_producer_stream(void *stream);
void *pixo_hip_get_producer_stream(void);   /* what the calling thread set (to save and restore it around a call) */
/* Releases the calling thread's device and pinned buffers AND every context parked by threads that have ended.
 * Buffers only grow while a thread lives; when it ends its context is parked for the next thread (no hipMalloc per
 * request in a thread-per-request server).  Parked contexts are bounded — at most 16 of them and 8 GiB of device +
 * pinned memory together, the oldest give their large buffers back first — but a LIVE thread keeps what its largest
 * image needed (a 16384x16384 image: ~2 GB of HBM, ~0.4 GB pinned) until it calls this. */
int pixo_hip_trim(void);
/* Tests and A/B tools only: replaces the debug switches read from the environment variable PIXO_HIP_DEBUG
 * ("name[=value],...": trace, host_entropy, multipass_entropy, direct_stores, one_piece, two_kernel_scan, fused_batch, no_side_stats, coef_form=scalar|packed, trellis_form=lane|group, batch_parts=n, png_batch_bytes=n, piece_groups=n, piece_medium=n,
 * piece_schedule=a:b:c, copy_threads=n, spin_budget=n, no_bands_upload, bands_upload_min_mb=n, bands_upload_mb=n — pixo_amd/csrc/capi_internal.hpp).  None of
 * them changes the bytes of a file.  NULL = read the environment again.  Not synchronised with calls in flight. */
int pixo_hip_debug_configure(const char *switches_or_null);
/* How often a single-pass entropy kernel gave up waiting (its waits on other workgroups are bounded) and the scan was
 * coded again by the multi-pass kernels, in this process.  0 in normal operation. */
uint64_t pixo_hip_debug_lookback_fallbacks(void);
/* Tests only: the set of internal routes (which kernel forms, stores and retries) that served calls in this process since the
 * record was last cleared, one bit per route (pixo_amd/csrc/capi_internal.hpp, namespace route; mirrored in pixo_amd/jpeg.py).
 * clear != 0: the record starts empty again.  Process-wide: calls of other threads show up too. */
uint64_t pixo_hip_debug_routes(int clear);
/* The dispatch gate of the single-pass kernels (pixo_amd/csrc/dispatch_gate.hpp: calls of several threads are kept from
 * starting such kernels on an empty device at the same moment — two launches that split the device's workgroup slots wait for
 * each other until the bounded waits give up): how often a launch found the launch before it, another thread's, not yet fully
 * dispatched and waited for it (*waits), and how often it stopped waiting after 5 ms (*timeouts).  Either pointer may be NULL. */
int pixo_hip_debug_dispatch_gate(uint64_t *waits, uint64_t *timeouts);
/* MEASUREMENT only (bench.py, tools/ab_binaries.py): a plain copy of `bytes` bytes of device memory in the coefficient
 * kernel's launch shape — one generation of 192-thread workgroups, 24 KiB each, 8 non-temporal 16-byte loads then 8
 * non-temporal stores per thread, no arithmetic (pixo_amd/csrc/stream_copy.hip) — so that a run can report what the
 * memory system of THIS box gives the kernel's 50 MB + 50 MB beside the kernel's own time.  Replaces nothing of the
 * reference.  `bytes` must be a multiple of 24576, the pointers 16-byte aligned; asynchronous on `stream`. */
int pixo_hip_debug_stream_copy(const void *d_in, void *d_out, size_t bytes, void *stream);
/* MEASUREMENT only: the same for a kernel that writes more or less than it reads — `workgroups` workgroups of 192 threads, every
 * thread `loads` non-temporal 16-byte loads, then `stores` non-temporal 16-byte stores (each in {1, 2, 4, 8, 16}): in = workgroups
 * x loads x 3072 bytes, out = workgroups x stores x 3072 bytes.  The 4:4:4 coefficient kernel is (tiles, 4, 8), the PNG filter
 * kernel (n, 8, 8), the fused pixel -> scan kernel on noise (tiles, 8, 2).  bench.py reports every kernel line beside it
 * (`copy_us_same_run`). */
int pixo_hip_debug_stream_io(const void *d_in, void *d_out, uint32_t workgroups, uint32_t loads, uint32_t stores, void *stream);
/* MEASUREMENT only: the engine clock in Hz while every SIMD issues vector instructions (four wavefronts each, ~1 ms of v_add_f32
 * chains; shader-clock ticks over constant-clock ticks).  The chip clocks down under vector load: bench.py puts a kernel's active
 * vector-ALU cycles over 1,024 SIMDs x THIS clock x the kernel's time (`frac_issue`), not over the 2.4 GHz peak.  Synchronises `stream`. */
int pixo_hip_debug_engine_clock(void *stream, double *hz);
/* MEASUREMENT only: the DEVICE work of one baseline file with standard tables — pixels -> the finished (stuffed, padded) scan in
 * the context's device buffer — enqueued on `stream` and NOT waited for; nothing is delivered.  The kernels are the ones
 * pixo_hip_jpeg_encode_device[_into] runs: the fused pixel -> scan kernel (jpeg_pixels_code.hip: ONE kernel; *form = 1) or
 * coefficient kernel + scan_code + stuffing kernel (*form = 0: gray images, debug switch two_kernel_scan).  K calls between
 * two events on `stream` = the device time per file without the call's waits and the file's way over PCIe.  The caller
 * synchronises the stream before it calls anything else of this library on the same thread. */
int pixo_hip_debug_scan_device_async(const void *d_pixels, const pixo_jpeg_options *options, void *stream, int *form);
/* ... the same for `batch` equally sized images back to back in device memory (configs[2]: 64 x 1920x1080) — the device work of
 * pixo_hip_jpeg_encode_batch_device[_into]'s one-pass form, the scans left in the context's device buffer at their files'
 * spacing: ONE launch of the fused kernel with every image a segment (*form = 1), or coefficient kernel + scan_code + stuffing
 * kernel over the batch (*form = 0).  batch = 1 is the entry above. */
int pixo_hip_debug_scan_device_async_batch(const void *d_pixels, const pixo_jpeg_options *options, uint32_t batch, void *stream, int *form);
/* Releases a buffer the library returned.  Blocks of 24 MiB and more are kept (at most two, 1 GiB) for the next large
 * file instead of going back to the system — their pages are resident, a fresh block of that size costs more than the
 * encode (profiles/r03_fresh_pages.txt); pixo_hip_trim() returns them. */
void pixo_hip_free(void *p);
/* memcpy of a finished file into storage of the caller's, by the library's copy threads (files of 2 MiB and more),
 * with a transparent-huge-page hint for a large destination that has not been touched yet.  For bindings that must
 * hand the file to their runtime in an object of the runtime's own (a Python bytes, a Java byte[]): the copy into a
 * fresh 178 MB object is 28 ms on one thread, 3 ms this way. */
void pixo_hip_copy_file(void *dst, const void *src, size_t n);
const char *pixo_hip_last_error(void);      /* thread-local, never NULL               */
const char *pixo_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXO_HIP_H */
