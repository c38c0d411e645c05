"""TEST HARNESS: a sequential model of baseline JPEG decode as libjpeg does it with its defaults — Huffman decode by the
standard (ITU T.81 F.2.2), the "islow" integer inverse DCT (jidctint), fancy h2v1 / h2v2 chroma upsampling (the triangle
filters with alternating rounding constants) and jdcolor's 16-bit fixed point.  Written from the algorithms, not from the
kernel: whole planes, Python integers and int64 arrays (nothing wraps), no tiles, no halo.  `decode(data)` gives
(width, height, pixels as a uint8 array, colour type 0 gray / 2 RGB); `coefficients(data)` the quantised coefficients per
component, zigzag order; `pixels(frame, coefficients)` is decode() behind the entropy decoder, for coefficients that were
never written to a file, and `unclamped(blocks)` the IDCT's samples in front of the clamp.  Refusals raise Refused(kind, message) with the library's words."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
INVALID, UNSUPPORTED = "Decode error: ", "Unsupported: "


class Refused(Exception):
    def __init__(self, kind, msg):
        super().__init__(kind + msg)
        self.kind, self.msg = kind, msg


class Frame:
    pass


def parse(d) -> Frame:
    """The marker walk up to SOS (only what the decode needs, and the refusals the tests of the model use)."""
    d = bytes(d)
    if len(d) < 2 or d[0] != 0xFF or d[1] != 0xD8:
        raise Refused(INVALID, "not a JPEG file")
    f = Frame()
    f.q, f.huff, f.restart, f.comps = {}, {}, 0, []
    p = 2
    while True:
        while p < len(d) and d[p] != 0xFF:
            p += 1
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d):
            raise Refused(INVALID, "unexpected end of file")
        m = d[p]
        p += 1
        if m == 0xD8 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise Refused(INVALID, "no image data found")
        if p + 2 > len(d):
            raise Refused(INVALID, "truncated marker")
        n = (d[p] << 8) | d[p + 1]
        if n < 2 or p + n > len(d):
            raise Refused(INVALID, "invalid marker length")
        s = d[p + 2:p + n]
        p += n
        if m == 0xC2:
            raise Refused(UNSUPPORTED, "progressive JPEG not supported")
        if m == 0xDB:
            o = 0
            while o < len(s):
                wide, t = s[o] >> 4, s[o] & 15
                o += 1
                if wide:
                    f.q[t] = [(s[o + 2 * i] << 8) | s[o + 2 * i + 1] for i in range(64)]
                    o += 128
                else:
                    f.q[t] = list(s[o:o + 64])
                    o += 64
        elif m == 0xC4:
            o = 0
            while o < len(s):
                key = (s[o] >> 4, s[o] & 15)
                bits = list(s[o + 1:o + 17])
                vals = list(s[o + 17:o + 17 + sum(bits)])
                o += 17 + sum(bits)
                code, k, table = 0, 0, {}
                for length in range(1, 17):
                    for _ in range(bits[length - 1]):
                        table[(length, code)] = vals[k]
                        k += 1
                        code += 1
                    code <<= 1
                f.huff[key] = table
        elif m == 0xC0:
            if s[0] != 8:
                raise Refused(UNSUPPORTED, "%d-bit precision not supported" % s[0])
            f.height, f.width = (s[1] << 8) | s[2], (s[3] << 8) | s[4]
            if s[5] not in (1, 3):
                raise Refused(UNSUPPORTED, "%d components not supported" % s[5])
            f.comps = [dict(id=s[6 + 3 * i], h=s[7 + 3 * i] >> 4, v=s[7 + 3 * i] & 15, tq=s[8 + 3 * i]) for i in range(s[5])]
        elif m == 0xDD:
            f.restart = (s[0] << 8) | s[1]
        elif m == 0xDA:
            for i in range(s[0]):
                f.comps[i]["td"], f.comps[i]["ta"] = s[2 + 2 * i] >> 4, s[2 + 2 * i] & 15
            if len(f.comps) == 1:
                f.comps[0]["h"] = f.comps[0]["v"] = 1  # a lone component's factors are ignored (T.81 A.2.2)
            f.scan = d[p:]
            return f


class _Bits:
    def __init__(self, d):
        self.d, self.p, self.b, self.n = d, 0, 0, 0

    def bit(self):
        if self.n == 0:
            if self.p >= len(self.d):
                raise Refused(INVALID, "entropy-coded segment ends early")
            x = self.d[self.p]
            self.p += 1
            if x == 0xFF:
                while self.p < len(self.d) and self.d[self.p] == 0xFF:
                    self.p += 1
                if self.p >= len(self.d) or self.d[self.p] != 0:
                    raise Refused(INVALID, "entropy-coded segment ends early")
                self.p += 1
            self.b, self.n = x, 8
        self.n -= 1
        return (self.b >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def restart(self, expected):
        self.n = 0
        while self.p + 1 < len(self.d) and self.d[self.p] == 0xFF and self.d[self.p + 1] == 0xFF:
            self.p += 1
        if not (self.p + 1 < len(self.d) and self.d[self.p] == 0xFF and self.d[self.p + 1] == 0xD0 + expected % 8):
            raise Refused(INVALID, "missing or out-of-sequence restart marker")
        self.p += 2


def _symbol(br, table):
    c = 0
    for length in range(1, 17):
        c = (c << 1) | br.bit()
        if (length, c) in table:
            return table[(length, c)]
    raise Refused(INVALID, "Huffman code not in the table")


def _extend(v, t):
    return v if t == 0 or v >= (1 << (t - 1)) else v - (1 << t) + 1


def coefficients(d):
    """(frame, [int64 array (blocks down, blocks across, 64) per component, zigzag order])"""
    f = parse(d)
    mh, mv = max(c["h"] for c in f.comps), max(c["v"] for c in f.comps)
    f.mh, f.mv = mh, mv
    f.mcus_x, f.mcus_y = -(-f.width // (8 * mh)), -(-f.height // (8 * mv))
    coefs = [np.zeros((f.mcus_y * c["v"], f.mcus_x * c["h"], 64), np.int64) for c in f.comps]
    br, pred, n, rst = _Bits(f.scan), [0] * len(f.comps), 0, 0
    for my in range(f.mcus_y):
        for mx in range(f.mcus_x):
            if f.restart and n and n % f.restart == 0:
                br.restart(rst)
                rst += 1
                pred = [0] * len(f.comps)
            for ci, c in enumerate(f.comps):
                for by in range(c["v"]):
                    for bx in range(c["h"]):
                        z = [0] * 64
                        t = _symbol(br, f.huff[(0, c["td"])])
                        pred[ci] += _extend(br.bits(t), t)
                        z[0] = pred[ci]
                        k = 1
                        while k < 64:
                            s = _symbol(br, f.huff[(1, c["ta"])])
                            if s & 15 == 0:
                                if s >> 4 != 15:
                                    break
                                k += 16
                                continue
                            k += s >> 4
                            if k > 63:
                                raise Refused(INVALID, "coefficient index past 63")
                            z[k] = _extend(br.bits(s & 15), s & 15)
                            k += 1
                        coefs[ci][my * c["v"] + by, mx * c["h"] + bx] = z
            n += 1
    return f, coefs


_C = dict(a=2446, b=3196, c=4433, d=6270, e=7373, f=9633, g=12299, h=15137, i=16069, j=16819, k=20995, l=25172)


def _idct8(d, shift):
    """jidctint's 8-point pass along axis -1 of an int64 array"""
    d = [d[..., i] for i in range(8)]
    z1 = (d[2] + d[6]) * _C["c"]
    t2, t3 = z1 - d[6] * _C["h"], z1 + d[2] * _C["d"]
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * _C["f"]
    t0, t1, t2, t3 = t0 * _C["a"], t1 * _C["j"], t2 * _C["l"], t3 * _C["g"]
    z1, z2, z3, z4 = z1 * -_C["e"], z2 * -_C["k"], z3 * -_C["i"] + z5, z4 * -_C["b"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([(x + r) >> shift for x in (t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3)], -1)


def dequantised(f, coefs, ci):
    """Component ci's blocks, dequantised, natural order: int64 (blocks down, blocks across, 8, 8)"""
    q = np.array(f.q[f.comps[ci]["tq"]], np.int64)
    nat = np.zeros(coefs[ci].shape, np.int64)
    nat[..., ZIGZAG] = coefs[ci] * q
    return nat.reshape(nat.shape[0], nat.shape[1], 8, 8)


def unclamped(blk):
    """Dequantised blocks (..., 8, 8) -> their descaled samples in front of the + 128 and the clamp"""
    ws = np.swapaxes(_idct8(np.swapaxes(blk, -1, -2), 11), -1, -2)  # columns
    return _idct8(ws, 18)                                            # rows


def plane(f, coefs, ci):
    """Component ci's padded plane of samples"""
    out = np.clip(unclamped(dequantised(f, coefs, ci)) + 128, 0, 255)
    by, bx = out.shape[:2]
    return out.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def _h2v1(p):
    """(rows, w) real samples -> (rows, 2w)"""
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def _h2v2(p):
    """(h, w) real samples -> (2h, 2w)"""
    above, below = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int64)
    for v, other in ((0, above), (1, below)):
        cs = 3 * p + other
        last, nxt = np.concatenate([cs[:, :1], cs[:, :-1]], 1), np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        out[v::2, 0::2] = (3 * cs + last + 8) >> 4
        out[v::2, 1::2] = (3 * cs + nxt + 7) >> 4
        out[v::2, 0], out[v::2, -1] = (cs[:, 0] * 4 + 8) >> 4, (cs[:, -1] * 4 + 7) >> 4
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def _rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb - _fix(0.71414) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(d):
    """(width, height, uint8 pixels (h, w) or (h, w, 3), colour type)"""
    return pixels(*coefficients(d))


def frame(width, height, comps, q):
    """The Frame of a file that was never written.  comps: [dict(h, v, tq)]; q: {id: 64 values in ZIGZAG order}"""
    f = Frame()
    f.width, f.height, f.comps, f.q = width, height, [dict(c) for c in comps], q
    if len(f.comps) == 1:
        f.comps[0]["h"] = f.comps[0]["v"] = 1
    return f


def pixels(f, coefs):
    """decode() behind the entropy decoder: coefs per component (blocks down, blocks across, 64), zigzag order"""
    W, H = f.width, f.height
    planes = [plane(f, coefs, ci) for ci in range(len(f.comps))]
    if len(f.comps) == 1:
        return W, H, planes[0][:H, :W].astype(np.uint8), 0
    factors = [(c["h"], c["v"]) for c in f.comps]
    if factors == [(1, 1)] * 3:
        up = planes
    elif factors in ([(2, 1), (1, 1), (1, 1)], [(2, 2), (1, 1), (1, 1)]) and -(-W // 2) <= 2:
        # jdsample.c chooses the fancy upsamplers only for more than two chroma samples a row; otherwise the nearest sample
        up = [planes[0]] + [np.repeat(np.repeat(p, factors[0][1], 0), 2, 1) for p in planes[1:]]
    elif factors == [(2, 1), (1, 1), (1, 1)]:
        up = [planes[0]] + [_h2v1(p[:H, :-(-W // 2)]) for p in planes[1:]]
    elif factors == [(2, 2), (1, 1), (1, 1)]:
        up = [planes[0]] + [_h2v2(p[:-(-H // 2), :-(-W // 2)]) for p in planes[1:]]
    else:
        raise Refused(UNSUPPORTED, "sampling factors %s not supported" % " ".join("%dx%d" % hv for hv in factors))
    return W, H, _rgb(*[u[:H, :W] for u in up]), 2
