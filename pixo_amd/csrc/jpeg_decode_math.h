// jpeg_decode_math.h — baseline JPEG decode behind the entropy decoder (jpeg_decode.hip): the coefficient layout the host writes
// and the kernel loads, dequantisation, the 8x8 inverse DCT, chroma upsampling, colour conversion, the crop, the record a
// workgroup reads and the tile -> image search.  The arithmetic is libjpeg's, restated: the "islow" integer IDCT (jidctint),
// the fancy h2v1 / h2v2 upsamplers (the 3:1 and 9:3:3:1 triangle filters with alternating rounding constants) and jdcolor's
// 16-bit fixed point, so that the pixels are byte for byte what libjpeg-turbo gives with its defaults.  Compiled for gfx950 by
// jpeg_decode.hip and for the HOST by the driver (jpeg_decode_api.cpp) and tests/emu_jpeg_decode: kernel, driver and emulation
// run the same code.  No HIP headers in here.
//
// EXTREME COEFFICIENTS.  Everything is 32-bit with unsigned wrap (no undefined behaviour) and the result is clamped to 0..255.
// libjpeg computes in `long` and indexes a masked range-limit table instead of clamping; the two agree as long as (a) no
// intermediate leaves 32 bits and (b) every descaled sample lies in -512..511.  No encoder of 8-bit pixels leaves either.
// Beyond (b) the samples here are the CLAMPED ones; libjpeg's C transform wraps there (its table is indexed modulo 1024), while
// a libjpeg-turbo with its SIMD transform was seen to saturate as this code does (lone coefficients with samples to +-1248).
// MEASURED against libjpeg-turbo (tests/jpeg_decode_arith.py, byte for byte): the largest lone dequantised coefficient that (b)
// allows — DC -4100 .. +4091; AC, either sign, from 2126 at (1, 1) to 4091 at (0, 4), (4, 0) and (4, 4) —, the same on DC +-1016,
// dense blocks at 0.6 .. 0.9 of the bound below, and files with their tables times 2 and times 4 (dequantised values to +-3768).
// With tables times 16 (values to +-15072, samples to +-2333) the pixels are still the clamped ones of 64-bit arithmetic, and
// 3 to 17 % of a file's bytes differ from libjpeg-turbo's.
// (a), derived.  One 8-point pass computes sums of products input x constant.  With a_k the sum of the constants' magnitudes
// that input k meets on its way to any intermediate of the pass,
//     a = {8192, 32501, 10703, 71869, 8192, 50643, 19570, 35521}        (k = 0..7; e.g. a_3 = 25172 + 20995 + 16069 + 9633)
// every intermediate of the column pass is at most sum_r a_r |d[r][c]| + 2^10 in magnitude, its outputs at most that / 2^11 + 1,
// and every intermediate of the row pass at most sum_c a_c |ws[r][c]| + 2^17.  With A_k = a_k / 8192 (1, 3.97, 1.31, 8.78, 1,
// 6.19, 2.39, 4.34) both passes stay inside 31 bits when
//     W(d) = sum over (r, c) of A_r * A_c * |d[r][c]|  <=  65000         (d: the DEQUANTISED block)
// — a sufficient bound, not a necessary one: a lone DC may reach 65000, a lone coefficient (3, 3) 843, while the measured cases
// above reach W = 163,000 (a lone (3, 3) of 2127) and, at tables times 16, W = 395,000 without an intermediate leaving 32 bits.
// within_bound() below evaluates it; the committed test files lie inside it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PIXO_JD_HD __host__ __device__ inline
#else
#define PIXO_JD_HD inline
#endif
#if defined(__clang__)
#define PIXO_JD_UNROLL _Pragma("unroll")
#else
#define PIXO_JD_UNROLL
#endif

namespace pixo_jdec {

enum { C_GRAY = 0, C_444 = 1, C_422 = 2, C_420 = 3, kClasses = 4 }; // one component; three with luma 1x1, 2x1, 2x2
enum { F_ALIGNED = 0, F_BYTES = 1, kForms = 2 };                    // the image starts at a multiple of 16 bytes; anywhere

// A workgroup of kWorkgroup lanes owns a tile of kTileMcusX x kTileMcusY whole MCUs of one image.
constexpr uint32_t kWorkgroup = 256;
constexpr uint32_t kTileMcusX = 16, kTileMcusY = 4;
constexpr uint64_t kMaxTiles = 0x7FFFFFFFull; // of one launch

PIXO_JD_HD constexpr uint32_t luma_h(int cls) { return cls >= C_422 ? 2u : 1u; } // luma blocks across / down an MCU
PIXO_JD_HD constexpr uint32_t luma_v(int cls) { return cls == C_420 ? 2u : 1u; }
PIXO_JD_HD constexpr uint32_t out_bpp(int cls) { return cls == C_GRAY ? 1u : 3u; }
// The planes of a tile in LDS.  Luma: the tile's own blocks.  Chroma of a subsampled class: a ring of one block around the
// tile's own in every subsampled direction — the upsampler reads one sample beyond the tile, and the block that holds it is
// transformed again by this workgroup (the halo).
PIXO_JD_HD constexpr uint32_t y_blocks_w(int cls) { return kTileMcusX * luma_h(cls); }
PIXO_JD_HD constexpr uint32_t y_blocks_h(int cls) { return kTileMcusY * luma_v(cls); }
PIXO_JD_HD constexpr uint32_t halo_x(int cls) { return luma_h(cls) - 1; }
PIXO_JD_HD constexpr uint32_t halo_y(int cls) { return luma_v(cls) - 1; }
PIXO_JD_HD constexpr uint32_t c_blocks_w(int cls) { return cls == C_GRAY ? 0u : kTileMcusX + 2 * halo_x(cls); }
PIXO_JD_HD constexpr uint32_t c_blocks_h(int cls) { return cls == C_GRAY ? 0u : kTileMcusY + 2 * halo_y(cls); }
PIXO_JD_HD constexpr uint32_t y_plane_bytes(int cls) { return y_blocks_w(cls) * y_blocks_h(cls) * 64; }
PIXO_JD_HD constexpr uint32_t c_plane_bytes(int cls) { return c_blocks_w(cls) * c_blocks_h(cls) * 64; }
PIXO_JD_HD constexpr uint32_t lds_bytes(int cls) { return y_plane_bytes(cls) + 2 * c_plane_bytes(cls); }
constexpr uint32_t kLdsBytesMax = 16384 + 2 * 6912; // C_420's: 30,208 bytes, five workgroups to a CU's 160 KiB
static_assert(lds_bytes(C_420) == kLdsBytesMax && lds_bytes(C_422) <= kLdsBytesMax && lds_bytes(C_444) <= kLdsBytesMax, "LDS budget");

// ---- the coefficient layout ---------------------------------------------------------------------------------------------------
// A component's blocks in raster order of its padded plane (mcus_x * h blocks a row), the count rounded up to 64.  Within a run
// of 64 blocks, row r (natural order) of all 64 blocks is contiguous: block b's row r is the 16 bytes at
// (b / 64) * 8192 + r * 1024 + (b % 64) * 16 — the r-th dwordx4 load of 64 lanes that hold 64 consecutive blocks covers 1 KiB.
PIXO_JD_HD uint64_t plane_blocks_padded(uint64_t blocks) { return (blocks + 63) & ~uint64_t{63}; }
PIXO_JD_HD uint64_t coef_index(uint64_t block, uint32_t natural) // in int16 units from the plane's start
{
    return (block >> 6) * 4096 + (natural >> 3) * 512 + (block & 63) * 8 + (natural & 7);
}

// ---- the record of an image in a launch ---------------------------------------------------------------------------------------
struct Record {
    uint64_t coef_at[3]; // bytes from the sub-batch's coefficients to each component's plane (multiples of 8192)
    uint64_t out_at;     // bytes from d_pixels to the image
    uint32_t width, height;
    uint32_t mcus_x, mcus_y;
    uint32_t tiles_x, tiles; // tiles across; tiles of the image
    uint32_t first_tile;     // the launch's tiles in front of this image
    uint32_t reserved;
    uint16_t q[3][64];       // the components' quantisation tables, natural order
};
static_assert(sizeof(Record) == 448 && sizeof(Record) % 16 == 0, "records are uploaded as they lie");

PIXO_JD_HD uint32_t tiles_x_of(uint32_t mcus_x) { return (mcus_x + kTileMcusX - 1) / kTileMcusX; }
PIXO_JD_HD uint32_t tiles_y_of(uint32_t mcus_y) { return (mcus_y + kTileMcusY - 1) / kTileMcusY; }

// The image whose tiles hold tile `t` of the launch: the last record with first_tile <= t (records are in launch order, none empty)
template <class R> PIXO_JD_HD uint32_t image_of_tile(const R *records, uint32_t count, uint32_t t)
{
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (records[mid].first_tile <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the inverse DCT ----------------------------------------------------------------------------------------------------------
// One 8-point pass of the islow IDCT: d[0..7] -> o[0..7], descaled by `shift` with rounding.  Unsigned arithmetic wraps.
PIXO_JD_HD int32_t descale(uint32_t x, int shift) { return (int32_t)(x + (1u << (shift - 1))) >> shift; }
PIXO_JD_HD void idct8(const int32_t *d, int32_t *o, int stride_in, int stride_out, int shift)
{
    const uint32_t d0 = (uint32_t)d[0], d1 = (uint32_t)d[stride_in], d2 = (uint32_t)d[2 * stride_in], d3 = (uint32_t)d[3 * stride_in];
    const uint32_t d4 = (uint32_t)d[4 * stride_in], d5 = (uint32_t)d[5 * stride_in], d6 = (uint32_t)d[6 * stride_in], d7 = (uint32_t)d[7 * stride_in];
    // even part
    uint32_t z1 = (d2 + d6) * 4433u;
    const uint32_t e2 = z1 - d6 * 15137u, e3 = z1 + d2 * 6270u;
    const uint32_t e0 = (d0 + d4) << 13, e1 = (d0 - d4) << 13;
    const uint32_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    // odd part
    uint32_t o0 = d7, o1 = d5, o2 = d3, o3 = d1;
    z1 = o0 + o3;
    uint32_t z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    o0 *= 2446u; o1 *= 16819u; o2 *= 25172u; o3 *= 12299u;
    z1 *= 0u - 7373u; z2 *= 0u - 20995u; z3 *= 0u - 16069u; z4 *= 0u - 3196u;
    z3 += z5; z4 += z5;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    o[0] = descale(t10 + o3, shift); o[7 * stride_out] = descale(t10 - o3, shift);
    o[stride_out] = descale(t11 + o2, shift); o[6 * stride_out] = descale(t11 - o2, shift);
    o[2 * stride_out] = descale(t12 + o1, shift); o[5 * stride_out] = descale(t12 - o1, shift);
    o[3 * stride_out] = descale(t13 + o0, shift); o[4 * stride_out] = descale(t13 - o0, shift);
}
PIXO_JD_HD uint32_t clamp255(int32_t v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }
// A dequantised block (natural order, in place) -> 64 samples: columns first (descale 13 - 2), then rows (13 + 2 + 3), + 128,
// clamp.  jidctint's shortcut for a column without AC terms gives the same values and is left out.
PIXO_JD_HD void idct_block(int32_t *blk)
{
PIXO_JD_UNROLL
    for (int c = 0; c < 8; ++c) idct8(blk + c, blk + c, 8, 8, 11);
PIXO_JD_UNROLL
    for (int r = 0; r < 8; ++r) {
        idct8(blk + 8 * r, blk + 8 * r, 1, 1, 18);
        PIXO_JD_UNROLL
        for (int c = 0; c < 8; ++c) blk[8 * r + c] = (int32_t)clamp255((int32_t)((uint32_t)blk[8 * r + c] + 128u));
    }
}
// The bound of the header comment on a dequantised block (natural order)
inline bool within_bound(const int32_t *d)
{
    static const double A[8] = {8192 / 8192.0, 32501 / 8192.0, 10703 / 8192.0, 71869 / 8192.0, 8192 / 8192.0, 50643 / 8192.0, 19570 / 8192.0, 35521 / 8192.0};
    double w = 0;
    for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 8; ++c) w += A[r] * A[c] * (d[8 * r + c] < 0 ? -(double)d[8 * r + c] : (double)d[8 * r + c]);
    return w <= 65000.0;
}

// ---- upsampling and colour ----------------------------------------------------------------------------------------------------
// jdcolor: FIX(1.402), FIX(1.772), FIX(0.34414), FIX(0.71414) at 16 bits; >> is arithmetic
PIXO_JD_HD void ycc_to_rgb(int32_t y, int32_t cb, int32_t cr, uint32_t *r, uint32_t *g, uint32_t *b)
{
    cb -= 128; cr -= 128;
    *r = clamp255(y + ((91881 * cr + 32768) >> 16));
    *g = clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    *b = clamp255(y + ((116130 * cb + 32768) >> 16));
}
// h2v1 fancy: sample `cur` with its neighbour on the output's side, even outputs round with 1, odd with 2
PIXO_JD_HD int32_t up_h2v1(int32_t cur, int32_t side, uint32_t x) { return (3 * cur + side + 1 + (int32_t)(x & 1)) >> 2; }
// h2v2 fancy: column sums 3 * near row + far row, of this column and of the neighbour on the output's side; 8 / 7
PIXO_JD_HD int32_t up_h2v2(int32_t this_sum, int32_t side_sum, uint32_t x) { return (3 * this_sum + side_sum + 8 - (int32_t)(x & 1)) >> 4; }

// ---- what a workgroup does ----------------------------------------------------------------------------------------------------
// The first MCU of tile `tile` of an image
template <int CLS, class R> PIXO_JD_HD void tile_geometry(const R *im, uint32_t tile, uint32_t *mx0, uint32_t *my0)
{
    *mx0 = (tile % im->tiles_x) * kTileMcusX;
    *my0 = (tile / im->tiles_x) * kTileMcusY;
}

// Phase A, lane `lane` of `lanes`: the blocks of the tile's planes, one block per lane and step.  coef: the sub-batch's
// coefficients.  lds: y plane, cb plane, cr plane (lds_bytes(CLS) bytes, 8-byte aligned).  Blocks outside the component's
// own grid (the tile's overhang at the right and bottom, the halo at the image's edges) are skipped; nothing reads them.
template <int CLS, class R>
PIXO_JD_HD void phase_a(const R *im, const uint8_t *coef, uint8_t *lds, uint32_t tile, uint32_t lane, uint32_t lanes)
{
    constexpr uint32_t YW = y_blocks_w(CLS), YH = y_blocks_h(CLS), CW = c_blocks_w(CLS), CH = c_blocks_h(CLS);
    constexpr uint32_t NY = YW * YH, NC = CW * CH;
    uint32_t mx0, my0;
    tile_geometry<CLS>(im, tile, &mx0, &my0);
    for (uint32_t t = lane; t < NY + 2 * NC; t += lanes) {
        uint32_t comp, pw, lx, ly; // component, its LDS plane's width in blocks, the block's place in that plane
        int64_t bx, by;            // ... and in the component's padded plane
        uint32_t comp_bw, comp_bh;
        uint8_t *plane;
        if (t < NY) {
            comp = 0; pw = YW; lx = t % YW; ly = t / YW;
            bx = (int64_t)mx0 * luma_h(CLS) + lx; by = (int64_t)my0 * luma_v(CLS) + ly;
            comp_bw = im->mcus_x * luma_h(CLS); comp_bh = im->mcus_y * luma_v(CLS);
            plane = lds;
        } else {
            constexpr uint32_t N = NC ? NC : 1, W = CW ? CW : 1; // (gray has no chroma blocks and never comes here)
            const uint32_t u = t - NY;
            comp = 1 + u / N; pw = CW; lx = (u % N) % W; ly = (u % N) / W;
            bx = (int64_t)mx0 + lx - halo_x(CLS); by = (int64_t)my0 + ly - halo_y(CLS);
            comp_bw = im->mcus_x; comp_bh = im->mcus_y;
            plane = lds + y_plane_bytes(CLS) + (comp - 1) * c_plane_bytes(CLS);
        }
        if (bx < 0 || by < 0 || bx >= (int64_t)comp_bw || by >= (int64_t)comp_bh) continue;
        const uint64_t b = (uint64_t)by * comp_bw + (uint64_t)bx;
        const uint8_t *src = coef + im->coef_at[comp] + (b >> 6) * 8192 + (b & 63) * 16;
        int32_t blk[64];
PIXO_JD_UNROLL
        for (int r = 0; r < 8; ++r) {
            typedef uint32_t Quad __attribute__((ext_vector_type(4)));
            const Quad v = *reinterpret_cast<const Quad *>(src + r * 1024);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            PIXO_JD_UNROLL
            for (int k = 0; k < 4; ++k) { // two int16 a word, little endian; the product wraps in 32 bits
                blk[8 * r + 2 * k] = (int32_t)((uint32_t)(int32_t)(int16_t)(w[k] & 0xFFFFu) * (uint32_t)im->q[comp][8 * r + 2 * k]);
                blk[8 * r + 2 * k + 1] = (int32_t)((uint32_t)(int32_t)(int16_t)(w[k] >> 16) * (uint32_t)im->q[comp][8 * r + 2 * k + 1]);
            }
        }
        idct_block(blk);
        uint32_t *dst = reinterpret_cast<uint32_t *>(plane + ((uint64_t)ly * 8 * pw + lx) * 8);
        PIXO_JD_UNROLL
        for (int r = 0; r < 8; ++r) {
            dst[r * pw * 2] = (uint32_t)blk[8 * r] | (uint32_t)blk[8 * r + 1] << 8 | (uint32_t)blk[8 * r + 2] << 16 | (uint32_t)blk[8 * r + 3] << 24;
            dst[r * pw * 2 + 1] = (uint32_t)blk[8 * r + 4] | (uint32_t)blk[8 * r + 5] << 8 | (uint32_t)blk[8 * r + 6] << 16 | (uint32_t)blk[8 * r + 7] << 24;
        }
    }
}

// One output pixel (x, y) of the image from the tile's planes: out[0..bpp)
template <int CLS, class R>
PIXO_JD_HD void pixel_of(const R *im, const uint8_t *lds, uint32_t mx0, uint32_t my0, uint32_t x, uint32_t y, uint32_t *out)
{
    constexpr uint32_t YPW = y_blocks_w(CLS) * 8, CPW = c_blocks_w(CLS) * 8;
    const uint32_t tx0 = mx0 * 8 * luma_h(CLS), ty0 = my0 * 8 * luma_v(CLS);
    const int32_t yy = lds[(y - ty0) * YPW + (x - tx0)];
    if (CLS == C_GRAY) { out[0] = (uint32_t)yy; return; }
    const uint8_t *cbp = lds + y_plane_bytes(CLS), *crp = cbp + c_plane_bytes(CLS);
    // the chroma planes' first sample, in chroma sample coordinates
    const int32_t pcx0 = ((int32_t)mx0 - (int32_t)halo_x(CLS)) * 8, pcy0 = ((int32_t)my0 - (int32_t)halo_y(CLS)) * 8;
    int32_t cb, cr;
    if (CLS == C_444) {
        const uint32_t at = (y - (uint32_t)pcy0) * CPW + (x - (uint32_t)pcx0);
        cb = cbp[at]; cr = crp[at];
    } else if (im->width <= 4) {
        // libjpeg takes its fancy upsamplers only for more than two chroma samples a row (jdsample.c: downsampled_width > 2);
        // a narrower image gets the nearest sample, in both directions
        const uint32_t at = ((CLS == C_420 ? y >> 1 : y) - (uint32_t)pcy0) * CPW + (uint32_t)((int32_t)(x >> 1) - pcx0);
        cb = cbp[at]; cr = crp[at];
    } else {
        // the real samples end at ceil(width / 2) (and ceil(height / 2)): beyond them the last one is replicated, as libjpeg does
        const int32_t cw = (int32_t)((im->width + 1) / 2);
        const int32_t cx = (int32_t)(x >> 1);
        int32_t sx = (x & 1) ? cx + 1 : cx - 1;
        sx = sx < 0 ? 0 : sx > cw - 1 ? cw - 1 : sx;
        if (CLS == C_422) {
            const uint32_t row = (y - (uint32_t)pcy0) * CPW;
            const uint32_t a = row + (uint32_t)(cx - pcx0), s = row + (uint32_t)(sx - pcx0);
            cb = up_h2v1(cbp[a], cbp[s], x); cr = up_h2v1(crp[a], crp[s], x);
        } else {
            const int32_t chh = (int32_t)((im->height + 1) / 2);
            const int32_t cy = (int32_t)(y >> 1);
            int32_t sy = (y & 1) ? cy + 1 : cy - 1;
            sy = sy < 0 ? 0 : sy > chh - 1 ? chh - 1 : sy;
            const uint32_t near_row = (uint32_t)(cy - pcy0) * CPW, far_row = (uint32_t)(sy - pcy0) * CPW;
            const uint32_t ca = (uint32_t)(cx - pcx0), cs = (uint32_t)(sx - pcx0);
            cb = up_h2v2(3 * cbp[near_row + ca] + cbp[far_row + ca], 3 * cbp[near_row + cs] + cbp[far_row + cs], x);
            cr = up_h2v2(3 * crp[near_row + ca] + crp[far_row + ca], 3 * crp[near_row + cs] + crp[far_row + cs], x);
        }
    }
    ycc_to_rgb(yy, cb, cr, &out[0], &out[1], &out[2]);
}

// Phase B, lane `lane` of `lanes`: the tile's pixels, cropped to the image.  The image is a flat run of width * height pixels;
// a lane takes groups of 16 pixels whose flat index starts at a multiple of 16 — in the aligned form such a group is bpp whole
// dwordx4 stores — and a row of the tile is cut into the groups it meets: a group the row fills is stored whole (F_ALIGNED)
// or byte by byte (F_BYTES); of a group the row shares with its neighbours only the row's own bytes are stored, one by one.
// out: d_pixels + out_at.
template <int CLS, int FORM, class R>
PIXO_JD_HD void phase_b(const R *im, const uint8_t *lds, uint8_t *out, uint32_t tile, uint32_t lane, uint32_t lanes)
{
    constexpr uint32_t BPP = out_bpp(CLS);
    constexpr uint32_t TW = kTileMcusX * 8 * luma_h(CLS), TH = kTileMcusY * 8 * luma_v(CLS);
    constexpr uint32_t GROUPS = TW / 16 + 1; // a row of at most TW pixels meets at most this many groups
    uint32_t mx0, my0;
    tile_geometry<CLS>(im, tile, &mx0, &my0);
    const uint32_t x0 = mx0 * 8 * luma_h(CLS), y0 = my0 * 8 * luma_v(CLS);
    const uint32_t x1 = im->width - x0 < TW ? im->width : x0 + TW, y1 = im->height - y0 < TH ? im->height : y0 + TH;
    if (x0 >= im->width || y0 >= im->height) return; // (a tile of padding only: an image whose MCUs overhang it by a tile — never, but cheap)
    const uint32_t rows = y1 - y0;
    for (uint32_t item = lane; item < rows * GROUPS; item += lanes) {
        const uint32_t y = y0 + item / GROUPS;
        const uint64_t p0 = (uint64_t)y * im->width + x0, p1 = (uint64_t)y * im->width + x1; // the row's flat pixels [p0, p1)
        const uint64_t g = p0 / 16 + item % GROUPS;
        if (g * 16 >= p1) continue;
        const uint64_t a = g * 16 < p0 ? p0 : g * 16, b = g * 16 + 16 > p1 ? p1 : g * 16 + 16;
        const uint32_t xa = (uint32_t)(a - (uint64_t)y * im->width);
        if (FORM == F_ALIGNED && b - a == 16) {
            uint32_t words[4 * BPP];
            PIXO_JD_UNROLL
            for (uint32_t k = 0; k < 4 * BPP; ++k) words[k] = 0;
            PIXO_JD_UNROLL
            for (uint32_t i = 0; i < 16; ++i) {
                uint32_t px[3];
                pixel_of<CLS>(im, lds, mx0, my0, xa + i, y, px);
                PIXO_JD_UNROLL
                for (uint32_t ch = 0; ch < BPP; ++ch) words[(i * BPP + ch) >> 2] |= px[ch] << (8 * ((i * BPP + ch) & 3));
            }
            typedef uint32_t Quad __attribute__((ext_vector_type(4)));
            Quad *dst = reinterpret_cast<Quad *>(out + a * BPP);
            PIXO_JD_UNROLL
            for (uint32_t k = 0; k < BPP; ++k) {
                Quad q;
                q.x = words[4 * k]; q.y = words[4 * k + 1]; q.z = words[4 * k + 2]; q.w = words[4 * k + 3];
                dst[k] = q;
            }
        } else {
            for (uint32_t i = 0; i < (uint32_t)(b - a); ++i) {
                uint32_t px[3];
                pixel_of<CLS>(im, lds, mx0, my0, xa + i, y, px);
                for (uint32_t ch = 0; ch < BPP; ++ch) out[(a + i) * BPP + ch] = (uint8_t)px[ch];
            }
        }
    }
}

} // namespace pixo_jdec
