// resize_math.h — the arithmetic of pixo::resize (reference src/resize.rs), one output pixel at a time, written once for
// the device kernels (resize.hip), for the host (the contribution tables, resize_api.cpp) and for the host build the tests
// drive (tests/emu_resize/).  Every f32 operation is rounded on its own: the library and the test harness are compiled
// with -ffp-contract=off, and nothing here may be re-associated.  Dimensions are at most 2^24, so every index is exact as
// an f32.
//
// The Lanczos weights need a sine.  The reference's wasm build carries Rust's `libm`, whose sinf is the musl / FreeBSD
// msun algorithm: argument reduced in f64, __sindf / __cosdf polynomials in f64, one rounding to f32 at the end.  The
// platform's sinf (glibc, the ROCm device library) differs from it in the last bit often enough to move output bytes, so
// rz_sinf below is that published algorithm, restated for |x| < 2^28 * pi/2 (the kernel argument never exceeds 3 pi).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define RZ_FN __host__ __device__ inline
#else
#define RZ_FN static inline
#endif

#define RZ_EPSILON 1.1920928955078125e-7f /* f32::EPSILON */
#define RZ_PI 3.14159274101257324f        /* std::f32::consts::PI */
#define RZ_MAX_DIMENSION (1u << 24)

enum { RZ_NEAREST = 0, RZ_BILINEAR = 1, RZ_LANCZOS3 = 2 };

// f32::round: halves away from zero.  x - trunc(x) is exact.
RZ_FN float rz_round(float x)
{
    const float t = truncf(x);
    if (fabsf(x - t) >= 0.5f) return t + copysignf(1.0f, x);
    return t;
}
// value.round().clamp(0.0, 255.0) as u8
RZ_FN uint8_t rz_to_u8(float v)
{
    float r = rz_round(v);
    r = r < 0.0f ? 0.0f : r;
    r = r > 255.0f ? 255.0f : r;
    return (uint8_t)r; // (a NaN cannot arise from finite weights and bytes)
}

// ---- nearest ------------------------------------------------------------------------------------------------------------
RZ_FN float rz_nearest_ratio(uint32_t src, uint32_t dst) { return (float)src / (float)dst; }
RZ_FN uint32_t rz_nearest_index(uint32_t d, float ratio, uint32_t src)
{
    float s = rz_round(((float)d + 0.5f) * ratio - 0.5f);
    s = s < 0.0f ? 0.0f : s;
    const float top = (float)(src - 1);
    s = s > top ? top : s;
    return (uint32_t)s;
}

// ---- bilinear -----------------------------------------------------------------------------------------------------------
RZ_FN float rz_bilinear_ratio(uint32_t src, uint32_t dst) { return dst > 1 ? (float)(src - 1) / (float)(dst - 1) : 0.0f; }
RZ_FN void rz_bilinear_axis(uint32_t d, float ratio, uint32_t src, uint32_t *i0, uint32_t *i1, float *frac)
{
    const float f = (float)d * ratio;
    const float fl = floorf(f);
    uint32_t a = (uint32_t)fl;
    // (f <= src - 1 up to one rounding of the product; an index past the last pixel would read outside the image, and the
    // reference would have panicked there: no golden case reaches it, the clamp only keeps the kernel inside its buffer)
    a = a > src - 1 ? src - 1 : a;
    *i0 = a;
    *i1 = a + 1 < src ? a + 1 : src - 1;
    *frac = f - (float)a;
}
RZ_FN uint8_t rz_bilinear_px(uint8_t p00, uint8_t p01, uint8_t p10, uint8_t p11, float fx, float fy)
{
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float top = (float)p00 * gx + (float)p01 * fx;
    const float bottom = (float)p10 * gx + (float)p11 * fx;
    return rz_to_u8(top * gy + bottom * fy);
}

// ---- the library's own sinf ------------------------------------------------------------------------------------------------
RZ_FN float rz_sindf(double x)
{
    const double S1 = -0x15555554cbac77.0p-55, S2 = 0x111110896efbb2.0p-59, S3 = -0x1a00f9e2cae774.0p-65, S4 = 0x16cd878c3b46a7.0p-71;
    const double z = x * x;
    const double w = z * z;
    const double r = S3 + z * S4;
    const double s = z * x;
    return (float)((x + s * (S1 + z * S2)) + s * w * r);
}
RZ_FN float rz_cosdf(double x)
{
    const double C0 = -0x1ffffffd0c5e81.0p-54, C1 = 0x155553e1053a42.0p-57, C2 = -0x16c087e80f1e27.0p-62, C3 = 0x199342e0ee5069.0p-68;
    const double z = x * x;
    const double w = z * z;
    const double r = C2 + z * C3;
    return (float)(((1.0 + z * C0) + w * C1) + (w * z) * r);
}
RZ_FN float rz_sinf(float x)
{
    const double pio2 = 1.57079632679489661923; // M_PI_2
    union { float f; uint32_t u; } b;
    b.f = x;
    const uint32_t ix = b.u & 0x7fffffffu;
    const bool neg = (b.u >> 31) != 0;
    if (ix <= 0x3f490fdau) { // |x| ~<= pi/4
        if (ix < 0x39800000u) return x; // |x| < 2^-12
        return rz_sindf(x);
    }
    if (ix <= 0x407b53d1u) { // |x| ~<= 5 pi/4
        if (ix <= 0x4016cbe3u) return neg ? -rz_cosdf((double)x + pio2) : rz_cosdf((double)x - pio2); // ~<= 3 pi/4
        return rz_sindf(neg ? -((double)x + 2 * pio2) : -((double)x - 2 * pio2));
    }
    if (ix <= 0x40e231d5u) { // |x| ~<= 9 pi/4
        if (ix <= 0x40afeddfu) return neg ? rz_cosdf((double)x + 3 * pio2) : -rz_cosdf((double)x - 3 * pio2); // ~<= 7 pi/4
        return rz_sindf(neg ? (double)x + 4 * pio2 : (double)x - 4 * pio2);
    }
    // the medium range of __rem_pio2f: n = nearest integer to x * 2/pi, y = x - n * pi/2 with pi/2 in two pieces
    const double toint = 6755399441055744.0; // 1.5 / DBL_EPSILON
    const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079631090164184570e+00, pio2_1t = 1.58932547735281966916e-08;
    const double fn = ((double)x * invpio2 + toint) - toint;
    const int n = (int)fn;
    const double y = ((double)x - fn * pio2_1) - fn * pio2_1t;
    switch (n & 3) {
    case 0: return rz_sindf(y);
    case 1: return rz_cosdf(y);
    case 2: return rz_sindf(-y);
    default: return -rz_cosdf(y);
    }
}

// ---- Lanczos3 -----------------------------------------------------------------------------------------------------------
// lanczos_kernel(x, 3.0)
RZ_FN float rz_lanczos3(float x)
{
    const float ax = fabsf(x);
    if (ax < RZ_EPSILON) return 1.0f;
    if (ax >= 3.0f) return 0.0f;
    const float pi_x = RZ_PI * x;
    const float pi_x_a = pi_x / 3.0f;
    return ((3.0f * rz_sinf(pi_x)) * rz_sinf(pi_x_a)) / (pi_x * pi_x_a);
}

// One axis of precompute_contributions: the taps of destination index d are source indices [start, end).
struct rz_axis {
    float scale, filter_scale, support;
};
RZ_FN rz_axis rz_axis_of(uint32_t src, uint32_t dst)
{
    rz_axis a;
    a.scale = (float)src / (float)dst;
    a.filter_scale = a.scale > 1.0f ? a.scale : 1.0f;
    a.support = 3.0f * a.filter_scale;
    return a;
}
RZ_FN float rz_center(const rz_axis a, uint32_t d) { return ((float)d + 0.5f) * a.scale - 0.5f; }
RZ_FN void rz_taps(const rz_axis a, uint32_t src, uint32_t d, uint32_t *start, uint32_t *end)
{
    const float c = rz_center(a, d);
    const float lo = floorf(c - a.support);
    *start = lo > 0.0f ? (uint32_t)lo : 0u; // (floor as isize).max(0)
    const float hi = ceilf(c + a.support);
    const uint64_t e = (hi > 0.0f ? (uint64_t)hi : 0u) + 1; // `as usize` saturates a negative float to 0
    *end = e < src ? (uint32_t)e : src;
}
// The normalised weights of destination index d into w[0 .. end - start).
RZ_FN void rz_weights(const rz_axis a, uint32_t d, uint32_t start, uint32_t end, float *w)
{
    const float c = rz_center(a, d);
    float sum = 0.0f;
    for (uint32_t s = start; s < end; ++s) {
        const float v = rz_lanczos3(((float)s - c) / a.filter_scale);
        w[s - start] = v;
        sum += v;
    }
    if (fabsf(sum) > RZ_EPSILON)
        for (uint32_t s = start; s < end; ++s) w[s - start] /= sum;
}
// one tap of one channel: sum += px as f32 * w (the product and the sum each rounded)
RZ_FN float rz_tap(float sum, uint8_t px, float w) { return sum + (float)px * w; }
