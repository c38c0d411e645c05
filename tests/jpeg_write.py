"""TEST HARNESS: a writer of baseline JPEG files (interleaved SOF0, one scan) from QUANTISED COEFFICIENTS, for the files no
encoder writes: any component ids, any assignment of quantisation and Huffman tables, tables of any legal shape, segments in
any order and grouping, fill bytes, redefined restart intervals, trailers, a missing EOI.  Written from the standard (ITU T.81:
F.1.2 the coding of a block, Annex C the code assignment, K.2 the optimal table); pure Python / numpy, nothing of this
library's encoder.  `write(...)` returns the file's bytes."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
DC, AC = 0, 1
EOB, ZRL = 0x00, 0xF0


# ---- Huffman tables: (BITS, HUFFVAL) = (16 counts, the symbols in code order) -------------------------------------------------
def table_from_lengths(lengths):
    """{symbol: code length 1..16} -> (BITS, HUFFVAL); the lengths must describe a prefix code (Kraft)"""
    assert lengths and all(1 <= n <= 16 for n in lengths.values())
    assert sum(1 << (16 - n) for n in lengths.values()) <= 1 << 16, "no prefix code has these lengths"
    order = sorted(lengths, key=lambda s: (lengths[s], s))
    bits = [0] * 16
    for s in order:
        bits[lengths[s] - 1] += 1
    return bits, order


def optimal_table(freq, reserve=True):
    """T.81 K.2: the optimal code for these symbol counts, lengths limited to 16.  `reserve`: keep the all-ones code word
    unused, as the standard's procedure does; without it the code is complete and its last code word is all ones."""
    used = sorted(s for s, n in freq.items() if n > 0)
    assert used
    if len(used) == 1 and not reserve:
        return table_from_lengths({used[0]: 1})
    f = [0] * 257
    for s in used:
        f[s] = freq[s]
    if reserve:
        f[256] = 1
    size, others = [0] * 257, [-1] * 257
    while True:
        live = [i for i in range(257) if f[i] > 0]
        if len(live) < 2:
            break
        v1 = min(live, key=lambda i: (f[i], -i))  # the least count, the largest symbol among equals
        v2 = min((i for i in live if i != v1), key=lambda i: (f[i], -i))
        f[v1] += f[v2]
        f[v2] = 0
        size[v1] += 1  # every symbol of both chains grows by a bit; v2's chain goes behind v1's
        while others[v1] != -1:
            v1 = others[v1]
            size[v1] += 1
        others[v1] = v2
        size[v2] += 1
        while others[v2] != -1:
            v2 = others[v2]
            size[v2] += 1
    bits = [0] * 34
    for i in range(257):
        if size[i]:
            bits[size[i]] += 1
    i = 32
    while i > 16:  # K.2 Adjust_BITS
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    if reserve:
        while bits[i] == 0:
            i -= 1
        bits[i] -= 1
    order = sorted(used, key=lambda s: (size[s], s))
    assert sum(bits[1:17]) == len(order)
    return bits[1:17], order


def long_codes_table(freq):
    """Every used symbol on a code of 9 to 16 bits: two symbols a length from 9 up, the rest at 16 (BITS 1..8 are zero)"""
    used = sorted((s for s, n in freq.items() if n > 0), key=lambda s: (-freq[s], s))
    return table_from_lengths({s: min(9 + i // 2, 16) for i, s in enumerate(used)})


def sixteen_bit_table(freq):
    """The optimal code, but the two rarest used symbols moved to 16 bits (the commonest too where there are few)"""
    bits, order = optimal_table(freq)
    lengths = dict(zip(order, [n + 1 for n in range(16) for _ in range(bits[n])]))
    rare = sorted(order, key=lambda s: (freq[s], s))[:2]
    for s in rare:
        lengths[s] = 16
    return table_from_lengths(lengths)


def codes_of(bits, vals):
    """Annex C: {symbol: (code, length)}"""
    out, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            assert code < 1 << n, "BITS describe no prefix code"
            out[vals[k]] = (code, n)
            code += 1
            k += 1
        code <<= 1
    return out


# ---- the scan --------------------------------------------------------------------------------------------------------------
def _magnitude(v):
    """F.1.2.1: (SSSS, the SSSS low bits that follow the code) of a DC difference or an AC coefficient"""
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v - 1) & ((1 << s) - 1)


def _block_symbols(z, pred, dc_key, ac_key, out):
    """One block (zigzag order): (table, symbol, extra bits, their count) appended to `out`"""
    s, x = _magnitude(z[0] - pred)
    assert s <= 11, "DC difference beyond category 11"
    out.append((dc_key, s, x, s))
    run = 0
    for k in range(1, 64):
        if z[k] == 0:
            run += 1
            continue
        while run > 15:
            out.append((ac_key, ZRL, 0, 0))
            run -= 16
        s, x = _magnitude(z[k])
        assert s <= 10, "AC coefficient beyond size 10"
        out.append((ac_key, (run << 4) | s, x, s))
        run = 0
    if run:
        out.append((ac_key, EOB, 0, 0))


def _pack(vals, lens):
    """Code words (uint64, most significant bit first, `lens` bits each) -> the entropy-coded bytes: padded with ones to a whole
    byte, a zero byte stuffed behind every 0xFF"""
    lens = np.asarray(lens, np.int64)
    vals = np.asarray(vals, np.uint64)
    ends = np.cumsum(lens)
    total = int(ends[-1]) if len(ends) else 0
    bits = np.ones((total + 7) // 8 * 8, np.uint8)
    starts = ends - lens
    for j in range(int(lens.max()) if len(lens) else 0):
        m = lens > j
        bits[starts[m] + j] = (vals[m] >> (lens[m] - 1 - j).astype(np.uint64)) & np.uint64(1)
    by = np.packbits(bits)
    return np.insert(by, np.flatnonzero(by == 255) + 1, 0).tobytes()


def _seg(marker, body):
    assert len(body) + 2 < 65536
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def write(width, height, comps, q, coefs, huff=None, restart=0, layout=None, q16=(), fill=None, rst_fill=None, trailer=b"", eoi=True, info=None):
    """The bytes of an interleaved baseline file.
    comps   [dict(id, h, v, tq, td, ta)] in frame (and scan) order, one or three
    q       {table id: 64 values, NATURAL order}; written with 16-bit entries where the id is in `q16` or a value needs it
    coefs   per component an integer array (blocks down, blocks across, 64) over its padded plane (whole MCUs), quantised,
            NATURAL order within a block
    huff    {(DC or AC, table id): (BITS, HUFFVAL) or a function of the table's symbol counts {symbol: n} that returns them};
            a table the components use and `huff` does not hold is optimal_table of its counts
    restart the interval of the default layout's DRI (0: none).  The scan follows the LAST DRI the layout holds.
    layout  the segments between SOI and the scan, in order: ("DQT", [id or (id, values, wide)...]), ("SOF",),
            ("DHT", [(class, id) or (class, id, (BITS, HUFFVAL))...]), ("DRI", interval), ("COM", bytes), ("SOS",) — the default:
            a DQT per table, SOF, a DHT per table, DRI where `restart`, SOS.  Tables given in place are decoys or redefinitions.
    fill    {index into layout, or "EOI": how many 0xFF fill bytes go in front of that marker}
    rst_fill  function of the restart marker's running number -> how many fill bytes go in front of it
    trailer bytes behind EOI; eoi=False leaves EOI out
    info    a dict that receives "huff" {(class, id): (BITS, HUFFVAL)} as written, "scan" (the entropy-coded bytes) and "symbols"
            {(class, id): {symbol: count}}"""
    huff = dict(huff or {})
    hmax, vmax = max(c["h"] for c in comps), max(c["v"] for c in comps)
    mcus_x, mcus_y = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    zz = []
    for c, a in zip(comps, coefs):
        a = np.asarray(a).astype(np.int64)
        assert a.shape == (mcus_y * c["v"], mcus_x * c["h"], 64), (a.shape, mcus_y, mcus_x)
        zz.append(a[..., ZIGZAG])
    if layout is None:
        layout = [("DQT", [t]) for t in sorted(q)] + [("SOF",)]
        keys = sorted({(DC, c["td"]) for c in comps} | {(AC, c["ta"]) for c in comps} | set(huff))
        layout += [("DHT", [k]) for k in keys] + ([("DRI", restart)] if restart else []) + [("SOS",)]
    interval = ([0] + [s[1] for s in layout if s[0] == "DRI"])[-1]

    # pass 1: the symbols, in scan order, cut at the restart intervals
    keys = sorted({(DC, c["td"]) for c in comps} | {(AC, c["ta"]) for c in comps})
    knum = {k: i for i, k in enumerate(keys)}
    if interval == 0 and all(not a[..., 1:].any() for a in zz):
        # every block is a DC difference and an end of block: the same symbols, vectorised
        dcs = [a[..., 0].reshape(mcus_y, c["v"], mcus_x, c["h"]).transpose(0, 2, 1, 3).reshape(mcus_y * mcus_x, -1) for c, a in zip(comps, zz)]
        tk, sym, xv, xl = [], [], [], []
        for c, d in zip(comps, dcs):
            flat = d.reshape(-1)
            diff = flat - np.concatenate([[0], flat[:-1]])
            s = np.zeros(diff.shape, np.int64)
            mag = np.abs(diff)
            for b in range(12):
                s += (mag >> b) > 0
            assert s.max() <= 11, "DC difference beyond category 11"
            x = np.where(diff >= 0, diff, diff - 1) & ((1 << s) - 1)
            shape = d.shape + (2,)
            tk.append(np.stack([np.full(d.shape, knum[(DC, c["td"])]), np.full(d.shape, knum[(AC, c["ta"])])], -1).reshape(shape))
            sym.append(np.stack([s.reshape(d.shape), np.full(d.shape, EOB)], -1))
            xv.append(np.stack([x.reshape(d.shape), np.zeros(d.shape, np.int64)], -1))
            xl.append(np.stack([s.reshape(d.shape), np.zeros(d.shape, np.int64)], -1))
        cat = lambda parts: np.concatenate([p.reshape(p.shape[0], -1) for p in parts], 1).reshape(-1)
        runs = [tuple(cat(p) for p in (tk, sym, xv, xl))]
    else:
        runs, cur, pred, n = [], [], [0] * len(comps), 0
        for my in range(mcus_y):
            for mx in range(mcus_x):
                if interval and n and n % interval == 0:
                    runs.append(cur)
                    cur, pred = [], [0] * len(comps)
                for ci, c in enumerate(comps):
                    for by in range(c["v"]):
                        for bx in range(c["h"]):
                            z = zz[ci][my * c["v"] + by, mx * c["h"] + bx].tolist()
                            _block_symbols(z, pred[ci], knum[(DC, c["td"])], knum[(AC, c["ta"])], cur)
                            pred[ci] = z[0]
                n += 1
        runs.append(cur)
        runs = [tuple(np.array([t[i] for t in r], np.int64) for i in range(4)) for r in runs]

    # the tables
    counts = {k: {} for k in keys}
    for tk, sym, _, _ in runs:
        for k in keys:
            s, n = np.unique(sym[tk == knum[k]], return_counts=True)
            for a, b in zip(s.tolist(), n.tolist()):
                counts[k][a] = counts[k].get(a, 0) + b
    for k in keys:
        t = huff.get(k, optimal_table)
        huff[k] = t(counts[k]) if callable(t) else t
    code, clen = np.zeros((len(keys), 256), np.uint64), np.zeros((len(keys), 256), np.int64)
    for k in keys:
        for s, (cw, n) in codes_of(*huff[k]).items():
            code[knum[k], s], clen[knum[k], s] = cw, n

    # pass 2: the bytes
    scan = b""
    for i, (tk, sym, xv, xl) in enumerate(runs):
        if i:
            scan += b"\xff" * (rst_fill(i - 1) if rst_fill else 0) + bytes([0xFF, 0xD0 + (i - 1) % 8])
        n = clen[tk, sym]
        assert n.all(), "a symbol in use has no code in its table"
        scan += _pack((code[tk, sym] << xl.astype(np.uint64)) | xv.astype(np.uint64), n + xl)

    # the segments
    def dqt(entry):
        t, values, wide = (entry, q[entry], entry in q16) if isinstance(entry, int) else entry
        values = [int(v) for v in np.asarray(values).reshape(64)]
        wide = wide or max(values) > 255
        assert 1 <= min(values) and max(values) < 65536
        return bytes([(16 if wide else 0) | t]) + b"".join(values[ZIGZAG[i]].to_bytes(2 if wide else 1, "big") for i in range(64))

    def dht(entry):
        bits, vals = huff[tuple(entry)] if len(entry) == 2 else entry[2]
        return bytes([(entry[0] << 4) | entry[1]]) + bytes(bits) + bytes(vals)

    out = b"\xff\xd8"
    fill = fill or {}
    for i, s in enumerate(layout):
        out += b"\xff" * fill.get(i, 0)
        if s[0] == "DQT":
            out += _seg(0xDB, b"".join(dqt(e) for e in s[1]))
        elif s[0] == "DHT":
            out += _seg(0xC4, b"".join(dht(e) for e in s[1]))
        elif s[0] == "SOF":
            out += _seg(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([len(comps)])
                        + b"".join(bytes([c["id"], (c["h"] << 4) | c["v"], c["tq"]]) for c in comps))
        elif s[0] == "DRI":
            out += _seg(0xDD, s[1].to_bytes(2, "big"))
        elif s[0] == "COM":
            out += _seg(0xFE, s[1])
        elif s[0] == "SOS":
            out += _seg(0xDA, bytes([len(comps)]) + b"".join(bytes([c["id"], (c["td"] << 4) | c["ta"]]) for c in comps) + bytes([0, 63, 0]))
        else:
            raise ValueError(s[0])
    assert layout[-1][0] == "SOS"
    if info is not None:
        info.update(huff={k: huff[k] for k in keys}, scan=scan, symbols=counts)
    return out + scan + (b"\xff" * fill.get("EOI", 0) + b"\xff\xd9" if eoi else b"") + bytes(trailer)


def gray(tq=0, td=0, ta=0, id=1):
    return [dict(id=id, h=1, v=1, tq=tq, td=td, ta=ta)]


def colour(mode, ids=(1, 2, 3), tq=(0, 1, 1), td=(0, 1, 1), ta=(0, 1, 1)):
    """Three components of "444", "422" or "420" """
    h, v = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}[mode]
    return [dict(id=ids[i], h=h if i == 0 else 1, v=v if i == 0 else 1, tq=tq[i], td=td[i], ta=ta[i]) for i in range(3)]
