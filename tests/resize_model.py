"""An independent numpy float32 model of pixo::resize, written from its contract (not shared with the product): vectorised over
pixels, a Python loop over taps, one rounding per f32 operation (numpy never fuses), the musl / FreeBSD sinf (argument reduction
and polynomials in f64, one rounding to f32).  Test harness only.

    nearest   ratio = src / dst;  index = clamp(round((d + 0.5) * ratio - 0.5), 0, src - 1), halves away from zero
    bilinear  ratio = (src - 1) / (dst - 1) or 0;  f = d * ratio, i0 = floor f, i1 = min(i0 + 1, src - 1), frac = f - i0
              value = (p00 (1 - fx) + p01 fx)(1 - fy) + (p10 (1 - fx) + p11 fx) fy
    lanczos3  horizontal pass into a u8 intermediate [src_h][dst_w], vertical pass; taps in order, one sum per channel
"""
import numpy as np

F = np.float32
EPS = F(1.1920928955078125e-07)
PI = F(3.14159274101257324)


def _round_away(x):
    t = np.trunc(x)
    return np.where(np.abs(x - t) >= F(0.5), t + np.copysign(F(1), x), t).astype(F)


def _to_u8(v):
    return np.clip(_round_away(v), F(0), F(255)).astype(np.uint8)


# ---- sinf -----------------------------------------------------------------------------------------------------------------
_S = [float.fromhex(h) for h in ("-0x15555554cbac77.0p-55", "0x111110896efbb2.0p-59", "-0x1a00f9e2cae774.0p-65", "0x16cd878c3b46a7.0p-71")]
_C = [float.fromhex(h) for h in ("-0x1ffffffd0c5e81.0p-54", "0x155553e1053a42.0p-57", "-0x16c087e80f1e27.0p-62", "0x199342e0ee5069.0p-68")]
_PIO2 = 1.57079632679489661923


def _sindf(x):
    z = x * x
    w = z * z
    r = _S[2] + z * _S[3]
    s = z * x
    return ((x + s * (_S[0] + z * _S[1])) + s * w * r).astype(F)


def _cosdf(x):
    z = x * x
    w = z * z
    r = _C[2] + z * _C[3]
    return (((1.0 + z * _C[0]) + w * _C[1]) + (w * z) * r).astype(F)


def sinf(x):
    """musl sinf for float32 arrays with |x| below 2^28 pi/2."""
    x = np.asarray(x, F)
    bits = x.view(np.uint32)
    ix = bits & np.uint32(0x7FFFFFFF)
    neg = (bits >> np.uint32(31)) != 0
    xd = x.astype(np.float64)
    sg = np.where(neg, 1.0, -1.0)  # x + k pi/2 for negative x, x - k pi/2 otherwise
    out = np.empty(x.shape, F)
    # general range first (overwritten below where a closer branch applies)
    fn = (xd * 6.36619772367581382433e-01 + 6755399441055744.0) - 6755399441055744.0
    n = fn.astype(np.int64) & 3
    y = (xd - fn * 1.57079631090164184570e+00) - fn * 1.58932547735281966916e-08
    out[:] = np.select([n == 0, n == 1, n == 2], [_sindf(y), _cosdf(y), _sindf(-y)], -_cosdf(y))
    m = ix <= 0x40E231D5  # <= 9 pi/4
    out[m] = np.where(ix <= 0x40AFEDDF, np.where(neg, _cosdf(xd + 3 * _PIO2), -_cosdf(xd - 3 * _PIO2)), _sindf(xd + sg * 4 * _PIO2))[m]
    m = ix <= 0x407B53D1  # <= 5 pi/4
    out[m] = np.where(ix <= 0x4016CBE3, np.where(neg, -_cosdf(xd + _PIO2), _cosdf(xd - _PIO2)), _sindf(-(xd + sg * 2 * _PIO2)))[m]
    m = ix <= 0x3F490FDA  # <= pi/4
    out[m] = np.where(ix < 0x39800000, x, _sindf(xd))[m]
    return out


# ---- Lanczos3 tables ------------------------------------------------------------------------------------------------------
def lanczos3(x):
    x = np.asarray(x, F)
    pi_x = PI * x
    pi_x_a = pi_x / F(3)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = ((F(3) * sinf(pi_x)) * sinf(pi_x_a)) / (pi_x * pi_x_a)
    ax = np.abs(x)
    return np.where(ax < EPS, F(1), np.where(ax >= F(3), F(0), v)).astype(F)


def contributions(src, dst):
    """(starts u32[dst], counts u32[dst], weights f32 packed end to end) of one axis."""
    scale = F(src) / F(dst)
    fs = max(scale, F(1))
    support = F(3) * fs
    d = np.arange(dst, dtype=np.int64)
    center = (d.astype(F) + F(0.5)) * scale - F(0.5)
    start = np.maximum(np.floor(center - support).astype(np.int64), 0)
    end = np.minimum(np.maximum(np.ceil(center + support).astype(np.int64), 0) + 1, src)
    counts = end - start
    weights = []
    for k in range(dst):  # (per destination index: the sum runs in tap order)
        s = np.arange(start[k], end[k], dtype=np.int64).astype(F)
        w = lanczos3((s - center[k]) / fs)
        total = F(0)
        for v in w:
            total = F(total + v)
        if abs(total) > EPS:
            w = (w / total).astype(F)
        weights.append(w)
    return start.astype(np.uint32), counts.astype(np.uint32), (np.concatenate(weights) if weights else np.zeros(0, F)).astype(F)


def _resample_axis0(img, src, dst):
    """img [src][...] u8 -> [dst][...] u8 along axis 0."""
    start, counts, w = contributions(src, dst)
    off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    acc = np.zeros((dst,) + img.shape[1:], F)
    shape = (dst,) + (1,) * (img.ndim - 1)
    for i in range(int(counts.max())):
        live = i < counts
        idx = np.minimum(start.astype(np.int64) + i, src - 1)
        wi = np.where(live, w[np.minimum(off[:-1] + i, len(w) - 1)], F(0)).astype(F)
        term = (img[idx].astype(F) * wi.reshape(shape)).astype(F)
        acc = np.where(live.reshape(shape), acc + term, acc).astype(F)
    return _to_u8(acc)


# ---- the three algorithms ----------------------------------------------------------------------------------------------------
def _nearest_index(src, dst):
    ratio = F(src) / F(dst)
    d = np.arange(dst).astype(F)
    return np.clip(_round_away((d + F(0.5)) * ratio - F(0.5)), F(0), F(src - 1)).astype(np.int64)


def _bilinear_axis(src, dst):
    ratio = F(src - 1) / F(dst - 1) if dst > 1 else F(0)
    f = (np.arange(dst).astype(F) * ratio).astype(F)
    i0 = np.floor(f).astype(np.int64)
    return i0, np.minimum(i0 + 1, src - 1), (f - i0.astype(F)).astype(F)


def resize(data, sw, sh, dw, dh, bpp, algorithm) -> bytes:
    img = np.ascontiguousarray(data, np.uint8).reshape(sh, sw, bpp)
    if algorithm == 0:
        return np.ascontiguousarray(img[_nearest_index(sh, dh)][:, _nearest_index(sw, dw)]).tobytes()
    if algorithm == 1:
        x0, x1, fx = _bilinear_axis(sw, dw)
        y0, y1, fy = _bilinear_axis(sh, dh)
        fx, fy = fx.reshape(1, dw, 1), fy.reshape(dh, 1, 1)
        gx, gy = F(1) - fx, F(1) - fy
        r0, r1 = img[y0].astype(F), img[y1].astype(F)
        top = r0[:, x0] * gx + r0[:, x1] * fx
        bottom = r1[:, x0] * gx + r1[:, x1] * fx
        return _to_u8(top * gy + bottom * fy).tobytes()
    if algorithm == 2:
        mid = _resample_axis0(np.ascontiguousarray(img.transpose(1, 0, 2)), sw, dw)  # [dw][sh][bpp]
        out = _resample_axis0(np.ascontiguousarray(mid.transpose(1, 0, 2)), sh, dh)   # [dh][dw][bpp]
        return out.tobytes()
    raise ValueError(algorithm)
