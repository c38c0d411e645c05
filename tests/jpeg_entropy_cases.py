"""TEST HARNESS for the device Huffman decode (PIXO_DECODE_DEVICE_ENTROPY): the host emulation's shim (tests/emu_jpeg_entropy_dec,
built on demand) and the files the tests write with tests/jpeg_write.py — borders of subsequences and workgroups, file ends, a
scan that never synchronises, malformed scans.  "Scan" is what the entry calls one: the bytes from behind SOS to the end of the
file, EOI and trailer included.  Everything is computed once and shared; nothing here needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

import jpeg_write as W

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_jpeg_entropy_dec")
MAIN = os.path.join(DIR, "jpeg_entropy_main")
VOUCHED, CHAIN_DEAD, NOT_SETTLED, SHORT, HOST = 0, 1, 2, 3, 4
_LIB = None
_cache = {}


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", DIR], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(DIR, "libpixo_emu_jpeg_entropy_dec.so"))
        L.emu_je_run.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_char_p]
        L.emu_je_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        L.emu_je_coef_values.argtypes = [C.c_void_p, C.c_size_t]
        L.emu_je_coef_values.restype = C.c_size_t
        _LIB = L
    return _LIB


def geometry():
    g = (C.c_uint32 * 5)()
    lib().emu_je_geometry(g)
    return dict(sub_bytes=g[0], group_subs=g[1], round_cap=g[2], min_scan_bytes=g[3], record_bytes=g[4])


def emulate(data, cap=0):
    """The passes on the host: dict(status 0 decoded / 1, 2 the walk refused / 3 the host's from the start, vouched, why, subs,
    rounds, launches, host_ok, coef (all components, the kernel's layout; None unless vouched), host_coef (None unless host_ok))"""
    buf = np.frombuffer(bytes(data), np.uint8)
    n = lib().emu_je_coef_values(buf.ctypes.data, buf.size)
    coef, host = np.zeros(max(n, 1), np.int16), np.zeros(max(n, 1), np.int16)
    info, msg = (C.c_uint32 * 6)(), C.create_string_buffer(256)
    rc = lib().emu_je_run(buf.ctypes.data, buf.size, cap, coef.ctypes.data, n, info, msg)
    host_ok = rc in (0, 3) and lib().emu_je_host(buf.ctypes.data, buf.size, host.ctypes.data, n) == 0
    return dict(status=rc, vouched=bool(info[0]) and rc == 0, why=info[1] if rc == 0 else HOST, subs=info[2], rounds=info[3], launches=info[4], host_ok=host_ok,
                coef=coef[:n] if rc == 0 and info[0] else None, host_coef=host[:n] if host_ok else None, msg=msg.value.decode())


def scan_of(data) -> bytes:
    """From behind SOS to the end of the file"""
    at = data.index(b"\xff\xda")
    return data[at + 2 + int.from_bytes(data[at + 2:at + 4], "big"):]


# ---- content ---------------------------------------------------------------------------------------------------------------
Q = {0: np.full(64, 3), 1: np.full(64, 5)}


def blocks(rng, bh, bw, dc=200, ac=40, density=0.15):
    """Quantised coefficients (bh, bw, 64), natural order: DCs that wander within +-dc, a share `density` of the ACs within +-ac"""
    a = np.zeros((bh, bw, 64), np.int64)
    a[..., 0] = rng.integers(-dc, dc + 1, (bh, bw))
    mask = rng.random((bh, bw, 63)) < density
    a[..., 1:] = np.where(mask, rng.integers(-ac, ac + 1, (bh, bw, 63)), 0)
    return a


def written(mode, w, h, seed, huff=None, info=None, **kw):
    """A file of random blocks: mode "gray", "444", "422" or "420"; kw: blocks()' and jpeg_write.write()'s"""
    rng = np.random.default_rng(seed)
    comps = W.gray() if mode == "gray" else W.colour(mode)
    hmax, vmax = max(c["h"] for c in comps), max(c["v"] for c in comps)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    content = {k: kw.pop(k) for k in ("dc", "ac", "density") if k in kw}
    coefs = [blocks(rng, my * c["v"], mx * c["h"], **content) for c in comps]
    return W.write(w, h, comps, Q if len(comps) == 3 else {0: Q[0]}, coefs, huff=huff, info=info, **kw)


def search(make, holds, seeds=range(400)):
    """The first seed's file for which holds(scan) is true"""
    for seed in seeds:
        data = make(seed)
        if holds(scan_of(data)):
            return data
    raise AssertionError("no seed gives the property")


def padded_to(data, scan_bytes):
    """The file with a trailer that makes its scan `scan_bytes` long"""
    have = len(scan_of(data))
    assert have <= scan_bytes, (have, scan_bytes)
    return data + bytes((7 * i + 1) & 0x7F for i in range(scan_bytes - have))


# fixed tables, so that a block's bits are known: the DC lengths of T.81's K.3 for categories 0..11, an end of block of one bit
_DC_LEN = {0: 2, 1: 3, 2: 3, 3: 3, 4: 3, 5: 3, 6: 4, 7: 5, 8: 6, 9: 7, 10: 8, 11: 9}
_FIXED = {(W.DC, 0): W.table_from_lengths(_DC_LEN), (W.AC, 0): W.table_from_lengths({0x00: 1})}


def exact_scan(scan_bytes, seed):
    """A gray file whose scan — entropy-coded data to its last byte, then EOI, no trailer — is exactly `scan_bytes` long: the
    first K blocks carry DC differences of categories 9 to 11, the blocks behind them repeat the last DC (three bits each); K by
    the bits the tables give, then K and the last difference varied until the stuffed bytes come out right."""
    rng = np.random.default_rng(seed)
    bw = 64 if scan_bytes > 4096 else 8
    bh = -(-(scan_bytes * 8 // 19) // bw) + 1  # (a rich block is 19 to 23 bits)
    n = bh * bw
    diffs = rng.choice([-1, 1], n) * rng.integers(256, 2048, n)
    diffs = np.where(np.abs(np.cumsum(diffs)) > 900, -np.abs(diffs) * np.sign(np.cumsum(diffs)), diffs)  # (roughly bounded; checked below)
    cat = np.array([int(abs(int(v))).bit_length() for v in diffs])
    bits = np.array([_DC_LEN[int(c)] for c in cat]) + cat + 1

    def file_of(k, last):
        d = diffs.copy()
        d[k - 1] = last
        d[k:] = 0
        dc = np.cumsum(d)
        a = np.zeros((bh, bw, 64), np.int64)
        a[..., 0] = dc.reshape(bh, bw)
        return W.write(bw * 8, bh * 8, W.gray(), {0: Q[0]}, [a], huff=_FIXED)
    want_bits = (scan_bytes - 2) * 8
    k = int(np.searchsorted(np.cumsum(bits) + 3 * (n - 1 - np.arange(n)), want_bits * 255 // 256))  # (one byte in 256 is stuffed)
    for _ in range(40):
        k = min(max(k, 2), n)
        for last in [int(diffs[k - 1])] + [s * (1 << c) for c in range(0, 11) for s in (1, -1)]:
            data = file_of(k, last)
            have = len(scan_of(data))
            if have == scan_bytes:
                return data
        k += (scan_bytes - have) * 8 // 18 or (1 if have < scan_bytes else -1)  # (a block that becomes rich grows by some 18 bits)
    raise AssertionError("no file with a scan of %d bytes" % scan_bytes)


def borders():
    """{name: file}: the border cases of the issue, by the emulation's geometry"""
    if "borders" in _cache:
        return _cache["borders"]
    g = geometry()
    S, G = g["sub_bytes"], g["group_subs"]
    gray = lambda seed, **kw: written("gray", 96, 64, seed, **kw)  # noqa: E731
    out = {}
    at_border = lambda s, off: any(s[k:k + 2] == b"\xff\x00" for k in range(S - off, len(s) - 4, S))  # noqa: E731
    rich = dict(dc=1000, ac=500, density=0.5)
    out["ff00_straddles_a_border"] = search(lambda seed: gray(seed, **rich), lambda s: at_border(s, 1))
    out["ff00_ends_at_a_border"] = search(lambda seed: gray(seed, **rich), lambda s: at_border(s, 2))
    # a block is 4 bytes (a DC code and an end of block of 16 bits each): every border is a block's end
    flat = [np.zeros((8, 12, 64), np.int64)]
    sixteen = {(W.DC, 0): W.table_from_lengths({0: 16}), (W.AC, 0): W.table_from_lengths({0: 16})}
    out["blocks_end_on_every_border"] = W.write(96, 64, W.gray(), {0: Q[0]}, flat, huff=sixteen)
    for n in (S - 1, S, S + 1, G * S - 1, G * S, G * S + 1):  # (entropy-coded data up to the scan's end, no trailer)
        out["scan_of_%d_bytes" % n] = exact_scan(n, n)
    three = written("420", 640, 480, 21, dc=1000, ac=300, density=0.45)
    assert 2 * G * S < len(scan_of(three)), len(scan_of(three))
    out["three_workgroups"] = padded_to(three, max(3 * G * S, len(scan_of(three)))) if len(scan_of(three)) <= 3 * G * S else three
    out["sixteen_bit_codes"] = written("444", 64, 48, 31, huff={(W.DC, 0): W.sixteen_bit_table, (W.AC, 0): W.sixteen_bit_table, (W.DC, 1): W.sixteen_bit_table,
                                                             (W.AC, 1): W.long_codes_table}, density=0.3)
    # every DC difference of category 11, every AC of size 10, no zero AC: whatever symbol crosses a border is one of them
    rng = np.random.default_rng(41)
    a = np.zeros((8, 12, 64), np.int64)
    a[..., 0] = np.where(np.arange(96).reshape(8, 12) % 2 == 0, 1000, -1000)
    a[..., 1:] = rng.choice([-1, 1], (8, 12, 63)) * rng.integers(512, 1024, (8, 12, 63))
    out["category_11_and_size_10_across_borders"] = W.write(96, 64, W.gray(), {0: Q[0]}, [a])
    out["stuffed_ff_is_the_last_scan_byte"] = search(lambda seed: gray(seed, **rich), lambda s: s[-4:] == b"\xff\x00\xff\xd9")
    out["fill_bytes_in_front_of_eoi"] = gray(51, fill={"EOI": 5})
    out["trailer"] = gray(52, trailer=bytes(range(1, 200)))
    out["no_eoi"] = gray(53, eoi=False)
    _cache["borders"] = out
    return out


def never_synchronises(subs):
    """A 4:2:0 file of all-zero blocks under single-symbol tables whose scan is all zero bits and about `subs` subsequences long.
    An MCU is 4 * (16 + 16) + (16 + 16) + (15 + 16) = 191 bits, a prime: a lane starts in step with the true decode only where a
    multiple of a subsequence's bits is a multiple of 191, that is every 191st lane, and a lane out of step stays out of step —
    every state of the decoder reads zero bits as a code of its table.  So with fewer than 191 subsequences round k repairs
    exactly subsequence k.  (The gray file of the issue has blocks of at most 32 bits: every 31st lane at the latest starts in
    step, and no such file needs more rounds than that.)"""
    key = ("never", subs)
    if key not in _cache:
        S = geometry()["sub_bytes"]
        mcus = subs * S * 8 // 191
        mx = 67
        my = -(-mcus // mx)
        comps = W.colour("420", td=(0, 0, 1), ta=(0, 0, 0))
        coefs = [np.zeros((my * c["v"], mx * c["h"], 64), np.int64) for c in comps]
        huff = {(W.DC, 0): W.table_from_lengths({0: 16}), (W.DC, 1): W.table_from_lengths({0: 15}), (W.AC, 0): W.table_from_lengths({0: 16})}
        _cache[key] = W.write(mx * 16, my * 16, comps, Q, coefs, huff=huff)
    return _cache[key]


def malformed():
    """{name: (file, the host's words or None)}: scans the host refuses"""
    if "malformed" in _cache:
        return _cache["malformed"]
    out = {}
    base = written("420", 96, 64, 61, density=0.3)
    head = len(base) - len(scan_of(base))
    for cut in (head + 40, head + 200, len(base) - 30):
        out["cut_at_%d" % (cut - head)] = (base[:cut], "entropy-coded segment ends early")
    # the optimal tables keep the all-ones word unused: sixteen ones in the scan start no code (unless they fall into value bits,
    # and then whatever the host says of what follows is the expectation)
    data = written("gray", 96, 64, 62, density=0.3)
    scan = bytearray(scan_of(data))
    scan[100:104] = b"\xff\x00\xff\x00"
    out["code_no_table_holds"] = (data[:len(data) - len(scan)] + bytes(scan), None)
    # sixty-two non-zero ACs and an end of block, the table's end of block then redefined as (run 1, size 1): index 64
    a = np.zeros((8, 12, 64), np.int64)
    a[..., 0] = 5
    a[..., W.ZIGZAG[1:63]] = 1
    dense = W.write(96, 64, W.gray(), {0: Q[0]}, [a], huff={(W.AC, 0): W.table_from_lengths({0x01: 1, 0x00: 2})})
    dht = bytes([0x10, 1, 1] + [0] * 14 + [0x01, 0x00])
    assert dense.count(dht) == 1
    out["index_past_63"] = (dense.replace(dht, dht[:-1] + b"\x11"), "coefficient index past 63")
    _cache["malformed"] = out
    return out
