// TEST HARNESS — the per-output-pixel resize arithmetic the device kernels run (pixo_amd/csrc/resize_math.h), compiled for
// the host and driven pixel by pixel in the kernels' order: the column terms once per column, Lanczos3 as two passes over a
// u8 intermediate with tables built once.
#include <cstdint>
#include <vector>

#include "../../pixo_amd/csrc/resize_math.h"

namespace {
struct Axis {
    std::vector<uint32_t> start, off;
    std::vector<float> w;
};
Axis build_axis(uint32_t src, uint32_t dst)
{
    Axis t;
    const rz_axis a = rz_axis_of(src, dst);
    t.start.resize(dst);
    t.off.resize(dst + 1);
    uint32_t at = 0;
    for (uint32_t d = 0; d < dst; ++d) {
        uint32_t s, e;
        rz_taps(a, src, d, &s, &e);
        t.start[d] = s;
        t.off[d] = at;
        t.w.resize(at + (e - s));
        rz_weights(a, d, s, e, t.w.data() + at);
        at += e - s;
    }
    t.off[dst] = at;
    return t;
}
} // namespace

extern "C" int emu_resize(const uint8_t *src, uint32_t sw, uint32_t sh, uint8_t *dst, uint32_t dw, uint32_t dh, uint32_t bpp, int algo)
{
    if (algo == RZ_NEAREST) {
        const float xr = rz_nearest_ratio(sw, dw), yr = rz_nearest_ratio(sh, dh);
        for (uint32_t y = 0; y < dh; ++y) {
            const size_t sy = rz_nearest_index(y, yr, sh);
            for (uint32_t x = 0; x < dw; ++x) {
                const size_t sx = rz_nearest_index(x, xr, sw);
                for (uint32_t c = 0; c < bpp; ++c) dst[((size_t)y * dw + x) * bpp + c] = src[(sy * sw + sx) * bpp + c];
            }
        }
        return 0;
    }
    if (algo == RZ_BILINEAR) {
        const float xr = rz_bilinear_ratio(sw, dw), yr = rz_bilinear_ratio(sh, dh);
        std::vector<uint32_t> x0(dw), x1(dw);
        std::vector<float> fx(dw);
        for (uint32_t x = 0; x < dw; ++x) rz_bilinear_axis(x, xr, sw, &x0[x], &x1[x], &fx[x]);
        for (uint32_t y = 0; y < dh; ++y) {
            uint32_t y0, y1;
            float fy;
            rz_bilinear_axis(y, yr, sh, &y0, &y1, &fy);
            const uint8_t *r0 = src + (size_t)y0 * sw * bpp, *r1 = src + (size_t)y1 * sw * bpp;
            for (uint32_t x = 0; x < dw; ++x)
                for (uint32_t c = 0; c < bpp; ++c)
                    dst[((size_t)y * dw + x) * bpp + c] = rz_bilinear_px(r0[(size_t)x0[x] * bpp + c], r0[(size_t)x1[x] * bpp + c],
                                                                         r1[(size_t)x0[x] * bpp + c], r1[(size_t)x1[x] * bpp + c], fx[x], fy);
        }
        return 0;
    }
    if (algo != RZ_LANCZOS3) return -1;
    const Axis h = build_axis(sw, dw), v = build_axis(sh, dh);
    const size_t row = (size_t)dw * bpp;
    std::vector<uint8_t> mid(row * sh);
    for (uint32_t y = 0; y < sh; ++y)
        for (uint32_t d = 0; d < dw; ++d)
            for (uint32_t c = 0; c < bpp; ++c) {
                float acc = 0.0f;
                for (uint32_t i = h.off[d]; i < h.off[d + 1]; ++i)
                    acc = rz_tap(acc, src[((size_t)y * sw + h.start[d] + (i - h.off[d])) * bpp + c], h.w[i]);
                mid[y * row + (size_t)d * bpp + c] = rz_to_u8(acc);
            }
    for (uint32_t y = 0; y < dh; ++y)
        for (size_t b = 0; b < row; ++b) {
            float acc = 0.0f;
            for (uint32_t i = v.off[y]; i < v.off[y + 1]; ++i) acc = rz_tap(acc, mid[(size_t)(v.start[y] + (i - v.off[y])) * row + b], v.w[i]);
            dst[y * row + b] = rz_to_u8(acc);
        }
    return 0;
}

extern "C" float emu_resize_sinf(float x) { return rz_sinf(x); }
