"""A reader of zlib / DEFLATE streams, written from RFC 1950 and RFC 1951 alone: it does not only inflate, it keeps what
the compressor decided — the blocks, their forms, their code lengths as written and every token with its bit offset and
width — and it raises on anything the format forbids.  Imports nothing of this library.  Test harness only."""
import struct

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8  # 288 symbols; 286 and 287 never occur
FIXED_DIST = [5] * 32                                   # 30 and 31 never occur
STORED, FIXED, DYNAMIC = 0, 1, 2


class FormatError(ValueError):
    """The stream is not valid zlib / DEFLATE."""


def length_symbol(length):
    """length 3..258 -> (symbol 257..285, extra bits)"""
    if length == 258:
        return 285, 0
    s = max(i for i in range(28) if LENGTH_BASE[i] <= length)
    return 257 + s, LENGTH_EXTRA[s]


def distance_symbol(dist):
    """distance 1..32768 -> (symbol 0..29, extra bits)"""
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, DIST_EXTRA[s]


def kraft(lens, limit=15):
    """Sum of 2^-len over the used symbols, scaled by 2^limit (a complete code: 2^limit)."""
    return sum(1 << (limit - l) for l in lens if l)


class Block:
    """final, btype; bit offsets start / first_token / end (from the first byte of the stream); for a dynamic block hlit,
    hdist, hclen, cl_lens (19, by symbol), runs [(code-length symbol, extra value)] as written, lit_lens (hlit entries),
    dist_lens (hdist entries); tokens [(position, length, distance) | (position, literal)] with offsets[] and widths[] in
    bits (a stored block has no tokens); out_start and data, the bytes it produces.  eob_offset / eob_width: the end-of-block
    symbol."""

    def __init__(self):
        self.final = self.btype = None
        self.start = self.first_token = self.end = None
        self.hlit = self.hdist = self.hclen = None
        self.cl_lens = self.runs = self.lit_lens = self.dist_lens = None
        self.tokens, self.offsets, self.widths = [], [], []
        self.eob_offset = self.eob_width = None
        self.out_start = 0
        self.data = b""


def _table(lens, what, allow_single=False):
    """lens -> (table indexed by the next `bits` bits of the stream, LSB first, entries sym << 4 | len or -1; bits)"""
    used = [l for l in lens if l]
    if not used:
        return None, 0
    top = max(used)
    k = kraft(lens, top)
    if k > (1 << top):
        raise FormatError("over-subscribed %s code" % what)
    if k < (1 << top) and not (allow_single and used == [1]):
        raise FormatError("incomplete %s code" % what)
    count = [0] * (top + 2)
    for l in used:
        count[l] += 1
    nxt, code = [0] * (top + 2), 0
    for b in range(1, top + 1):
        code = (code + count[b - 1]) << 1 if b > 1 else 0
        nxt[b] = code
    table = [-1] * (1 << top)
    for sym, l in enumerate(lens):
        if l:
            c = nxt[l]
            nxt[l] += 1
            rev = int(format(c, "0%db" % l)[::-1], 2)
            n = 1 << (top - l)
            table[rev::1 << l] = [sym << 4 | l] * n
    return table, top


class _Bits:
    def __init__(self, buf):
        self.buf, self.pos, self.total = buf, 0, 8 * len(buf)

    def get(self, n):
        if self.pos + n > self.total:
            raise FormatError("the stream ends inside a block")
        byte, sh = self.pos >> 3, self.pos & 7
        v = (int.from_bytes(self.buf[byte:byte + 4], "little") >> sh) & ((1 << n) - 1)  # n <= 16
        self.pos += n
        return v

    def symbol(self, table, bits, what):
        byte, sh = self.pos >> 3, self.pos & 7
        e = table[(int.from_bytes(self.buf[byte:byte + 4], "little") >> sh) & ((1 << bits) - 1)]
        if e < 0:
            raise FormatError("a bit pattern that is no %s code" % what)
        self.pos += e & 15
        if self.pos > self.total:
            raise FormatError("the stream ends inside a block")
        return e >> 4


def _dynamic_header(b, r):
    b.hlit, b.hdist, b.hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
    if b.hlit > 286 or b.hdist > 30:
        raise FormatError("HLIT %d / HDIST %d: more symbols than the alphabets have" % (b.hlit, b.hdist))
    b.cl_lens = [0] * 19
    for i in range(b.hclen):
        b.cl_lens[CL_ORDER[i]] = r.get(3)
    table, bits = _table(b.cl_lens, "code-length")
    if table is None:
        raise FormatError("no code-length code")
    lens, b.runs = [], []
    total = b.hlit + b.hdist
    while len(lens) < total:
        s = r.symbol(table, bits, "code-length")
        if s < 16:
            b.runs.append((s, 0))
            lens.append(s)
            continue
        extra = r.get({16: 2, 17: 3, 18: 7}[s])
        b.runs.append((s, extra))
        if s == 16:
            if not lens:
                raise FormatError("a repeat with no length before it")
            lens += [lens[-1]] * (3 + extra)
        else:
            lens += [0] * ((3 if s == 17 else 11) + extra)
    if len(lens) > total:
        raise FormatError("a run of code lengths goes past HLIT + HDIST")
    b.lit_lens, b.dist_lens = lens[:b.hlit], lens[b.hlit:]
    if not b.lit_lens[256]:
        raise FormatError("no end-of-block code")


def read_deflate(buf, bit_start=0, history=b""):
    """The DEFLATE blocks of buf from bit offset bit_start up to the final one -> (blocks, bit offset of the end, output).
    `history`: bytes a distance may reach back into (they are not part of the output returned)."""
    r = _Bits(buf)
    r.pos = bit_start
    out = bytearray(history)
    skip = len(history)
    blocks = []
    while True:
        b = Block()
        b.start = r.pos
        b.final = r.get(1)
        b.btype = r.get(2)
        b.out_start = len(out) - skip
        if b.btype == 3:
            raise FormatError("block type 3")
        if b.btype == STORED:
            pad = (-r.pos) & 7
            if r.get(pad):
                raise FormatError("non-zero padding bits before a stored block")
            n, nn = r.get(16), r.get(16)
            if n ^ nn != 0xFFFF:
                raise FormatError("NLEN is not the complement of LEN")
            b.first_token = r.pos
            if r.pos + 8 * n > r.total:
                raise FormatError("the stream ends inside a stored block")
            out += buf[r.pos >> 3:(r.pos >> 3) + n]
            r.pos += 8 * n
        else:
            if b.btype == DYNAMIC:
                _dynamic_header(b, r)
                lit_lens, dist_lens = b.lit_lens, b.dist_lens
            else:
                lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
            lt, lb = _table(lit_lens, "literal/length")
            dt, db = _table(dist_lens, "distance", allow_single=True)
            b.first_token = r.pos
            _tokens(b, r, out, skip, lt, lb, dt, db)
        b.end = r.pos
        b.data = bytes(out[skip + b.out_start:])
        blocks.append(b)
        if b.final:
            return blocks, r.pos, bytes(out[skip:])


def _tokens(b, r, out, skip, lt, lb, dt, db):
    """The symbols of a fixed or dynamic block up to its end-of-block symbol (the inner loop: bits kept in an integer)."""
    buf, total = r.buf, r.total
    pos = r.pos
    byte = pos >> 3
    acc = int.from_bytes(buf[byte:byte + 8], "little") >> (pos & 7)
    cnt = 64 - (pos & 7)
    byte += 8
    lmask, dmask = (1 << lb) - 1, (1 << db) - 1
    tokens, offsets, widths = b.tokens, b.offsets, b.widths
    while True:
        while cnt < 48:  # a token has at most 48 bits
            acc |= int.from_bytes(buf[byte:byte + 4], "little") << cnt
            byte += 4
            cnt += 32
        e = lt[acc & lmask]
        if e < 0:
            raise FormatError("a bit pattern that is no literal/length code")
        k = e & 15
        sym = e >> 4
        if sym < 256:
            tokens.append((len(out) - skip, sym))
            offsets.append(pos)
            widths.append(k)
            out.append(sym)
            acc >>= k
            cnt -= k
            pos += k
            if pos > total:
                raise FormatError("the stream ends inside a block")
            continue
        if sym == 256:
            b.eob_offset, b.eob_width = pos, k
            pos += k
            if pos > total:
                raise FormatError("the stream ends inside a block")
            r.pos = pos
            return
        if sym > 285:
            raise FormatError("literal/length symbol %d" % sym)
        width = k
        acc >>= k
        eb = LENGTH_EXTRA[sym - 257]
        length = LENGTH_BASE[sym - 257] + (acc & ((1 << eb) - 1))
        acc >>= eb
        width += eb
        if dt is None:
            raise FormatError("a match in a block with no distance code")
        e = dt[acc & dmask]
        if e < 0:
            raise FormatError("a bit pattern that is no distance code")
        k = e & 15
        ds = e >> 4
        if ds > 29:
            raise FormatError("distance symbol %d" % ds)
        acc >>= k
        eb = DIST_EXTRA[ds]
        dist = DIST_BASE[ds] + (acc & ((1 << eb) - 1))
        acc >>= eb
        width += k + eb
        if pos + width > total:
            raise FormatError("the stream ends inside a block")
        if dist > len(out):
            raise FormatError("a distance of %d at output position %d: before the start of the stream" % (dist, len(out) - skip))
        tokens.append((len(out) - skip, length, dist))
        offsets.append(pos)
        widths.append(width)
        if dist >= length:
            out += out[len(out) - dist:len(out) - dist + length]
        else:
            for _ in range(length):
                out.append(out[-dist])
        cnt -= width
        pos += width


class ZlibStream:
    """header (2 bytes), adler32 (as written), blocks, data (all output), end (bit offset behind the last block)"""


def read_zlib(stream):
    stream = bytes(stream)
    if len(stream) < 6:
        raise FormatError("shorter than a zlib header and trailer")
    z = ZlibStream()
    z.header = stream[:2]
    if (z.header[0] & 15) != 8 or (z.header[0] >> 4) > 7 or (z.header[0] * 256 + z.header[1]) % 31 or z.header[1] & 32:
        raise FormatError("not a zlib header without a preset dictionary")
    z.blocks, z.end, z.data = read_deflate(stream[:-4], 16)
    if (z.end + 7) // 8 != len(stream) - 4:
        raise FormatError("%d bytes between the last block and the checksum" % (len(stream) - 4 - (z.end + 7) // 8))
    z.adler32 = struct.unpack(">I", stream[-4:])[0]
    return z


def token_bytes(tokens, history=b""):
    """The bytes a token list stands for (positions are not looked at)."""
    out = bytearray(history)
    for t in tokens:
        if len(t) == 2:
            out.append(t[1])
        else:
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out[len(history):])
