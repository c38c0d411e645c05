// png_inflate.cpp — DEFLATE decoding on the host (RFC 1951) as the reference does it (src/decode/inflate.rs, bit_reader.rs):
// a 9-bit lookup table per code with a bit-by-bit walk for longer codes, the same table for ill-formed code sets (later
// symbols overwrite earlier ones, as from_lengths fills it), the same order of checks and the same messages.  Decoding is
// sequential; the device takes over behind it (png_unfilter.hip).
#include "png_inflate.hpp"

#include <cstring>

namespace pixo_inflate {

namespace {

const uint16_t kLengthBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t kLengthExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
const uint8_t kCodeLengthOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
constexpr unsigned kMaxBits = 15, kLookupBits = 9;
constexpr size_t kWindow = 32768;

const char *const kEnd = "unexpected end of stream";

// BitReader (bit_reader.rs:10-116), LSB first.  The buffer is refilled eight bytes at a time; what the reference's byte-wise
// reader can see — how many bits are left in all — is the same.
struct Bits {
    const uint8_t *p;
    size_t n, pos = 0;
    uint64_t buf = 0;
    unsigned cnt = 0;
    Bits(const uint8_t *data, size_t len) : p(data), n(len) {}
    void refill()
    {
        if (pos + 8 <= n) {
            uint64_t w;
            std::memcpy(&w, p + pos, 8); // (little-endian hosts only, as the rest of the library)
            buf |= w << cnt;
            pos += (63 - cnt) >> 3;
            cnt |= 56;
        } else
            while (cnt <= 56 && pos < n) {
                buf |= static_cast<uint64_t>(p[pos++]) << cnt;
                cnt += 8;
            }
    }
    bool need(unsigned k)
    {
        if (cnt < k) refill();
        return cnt >= k;
    }
    uint32_t peek(unsigned k) const { return static_cast<uint32_t>(buf & ((uint64_t{1} << k) - 1)); }
    void consume(unsigned k) { buf >>= k; cnt -= k; }
    bool read(unsigned k, uint32_t *v)
    {
        if (!need(k)) return false;
        *v = peek(k);
        consume(k);
        return true;
    }
    void align() { consume(cnt % 8); }
};

// The output: `cap` bytes of the caller's, and behind them a 32 KiB ring that only later matches read.
struct Sink {
    uint8_t *out;
    size_t cap, n = 0;
    uint32_t over_adler = 1; // the checksum once the stream has outgrown `cap`
    uint8_t ring[kWindow];
    Sink(uint8_t *o, size_t c) : out(o), cap(c) {}
    uint8_t at(size_t i) const { return i < cap ? out[i] : ring[(i - cap) & (kWindow - 1)]; }
    void put(uint8_t b)
    {
        if (n < cap) out[n] = b;
        else {
            if (n == cap) over_adler = adler32(out, cap);
            ring[(n - cap) & (kWindow - 1)] = b;
            over_adler = adler32(&b, 1, over_adler);
        }
        ++n;
    }
    uint32_t adler() const { return n > cap ? over_adler : adler32(out, n); }
};

// HuffmanTable (inflate.rs:46-220)
struct Huff {
    uint16_t lookup[1u << kLookupBits];
    uint32_t first[kMaxBits + 1]; // the code of the first symbol of every length
    uint16_t count[kMaxBits + 1], offset[kMaxBits + 1], sorted[320];
    unsigned max_len = 0;

    void build(const uint8_t *lengths, size_t symbols) // (no length exceeds 15: they come from 4-bit symbols)
    {
        std::memset(lookup, 0, sizeof lookup);
        std::memset(count, 0, sizeof count);
        max_len = 0;
        for (size_t s = 0; s < symbols; ++s) {
            if (lengths[s] > max_len) max_len = lengths[s];
            if (lengths[s]) ++count[lengths[s]];
        }
        if (!max_len) return;
        uint32_t code = 0, next[kMaxBits + 1];
        uint16_t at = 0;
        first[0] = 0;
        offset[0] = 0;
        for (unsigned bits = 1; bits <= kMaxBits; ++bits) {
            code = (code + (bits > 1 ? count[bits - 1] : 0u)) << 1;
            first[bits] = next[bits] = code;
            offset[bits] = at;
            at = static_cast<uint16_t>(at + count[bits]);
        }
        uint16_t fill[kMaxBits + 1] = {};
        for (size_t s = 0; s < symbols; ++s) {
            const unsigned len = lengths[s];
            if (!len) continue;
            const uint32_t c = next[len]++;
            sorted[offset[len] + fill[len]++] = static_cast<uint16_t>(s);
            if (len > kLookupBits) continue;
            uint32_t reversed = 0, v = c & 0xFFFFu;
            for (unsigned i = 0; i < len; ++i) { reversed = (reversed << 1) | (v & 1); v >>= 1; }
            for (uint32_t i = 0; i < (1u << (kLookupBits - len)); ++i)
                lookup[reversed | (i << len)] = static_cast<uint16_t>(s | (len << 12));
        }
    }
    // decode (inflate.rs:130-186); null: *err says why
    bool decode(Bits &r, uint32_t *symbol, const char **err) const
    {
        if (!max_len) { *err = "empty Huffman table"; return false; }
        r.need(kLookupBits);
        const unsigned avail = r.cnt < kLookupBits ? r.cnt : kLookupBits;
        if (avail) {
            const uint16_t e = lookup[r.peek(avail)];
            const unsigned len = e >> 12;
            if (len && len <= avail) {
                r.consume(len);
                *symbol = e & 0xFFFu;
                return true;
            }
        }
        uint32_t code = 0;
        for (unsigned len = 1; len <= max_len; ++len) {
            uint32_t bit;
            if (!r.read(1, &bit)) { *err = kEnd; return false; }
            code = (code << 1) | bit;
            if (code >= first[len] && code - first[len] < count[len]) {
                *symbol = sorted[offset[len] + (code - first[len])];
                return true;
            }
        }
        *err = "invalid Huffman code";
        return false;
    }
};

struct FixedTables {
    Huff lit, dist;
    FixedTables()
    {
        uint8_t l[288], d[32];
        for (int i = 0; i < 288; ++i) l[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
        std::memset(d, 5, sizeof d);
        lit.build(l, 288);
        dist.build(d, 32);
    }
};

struct Inflater {
    Bits r;
    Sink &o;
    std::string err;
    Inflater(const uint8_t *d, size_t n, Sink &s) : r(d, n), o(s) {}
    bool fail(const char *m) { err = m; return false; }

    bool stored() // inflate_stored (:355-376)
    {
        r.align();
        uint32_t len, nlen;
        if (!r.read(16, &len) || !r.read(16, &nlen)) return fail(kEnd);
        if (len != ((~nlen) & 0xFFFFu)) return fail("stored block LEN/NLEN mismatch");
        if (len > r.cnt / 8 + (r.n - r.pos)) return fail(kEnd);
        for (uint32_t i = 0; i < len; ++i) {
            if (r.cnt) { o.put(static_cast<uint8_t>(r.peek(8))); r.consume(8); }
            else {
                const size_t run = len - i; // the buffer is empty: the rest comes straight from the input
                r.buf = 0;                  // (a refill leaves the bits of the next bytes above `cnt`)
                if (o.n + run <= o.cap) { std::memcpy(o.out + o.n, r.p + r.pos, run); o.n += run; }
                else for (size_t k = 0; k < run; ++k) o.put(r.p[r.pos + k]);
                r.pos += run;
                break;
            }
        }
        return true;
    }
    bool block(const Huff &lit, const Huff &dist) // inflate_block (:461-513)
    {
        const char *e = nullptr;
        for (;;) {
            uint32_t sym;
            if (!lit.decode(r, &sym, &e)) return fail(e);
            if (sym < 256) { o.put(static_cast<uint8_t>(sym)); continue; }
            if (sym == 256) return true;
            if (sym > 285) { err = "invalid literal/length code: " + std::to_string(sym); return false; }
            uint32_t extra, dsym;
            if (!r.read(kLengthExtra[sym - 257], &extra)) return fail(kEnd);
            const size_t length = kLengthBase[sym - 257] + extra;
            if (!dist.decode(r, &dsym, &e)) return fail(e);
            if (dsym >= 30) return fail("invalid distance code");
            if (!r.read(kDistExtra[dsym], &extra)) return fail(kEnd);
            const size_t distance = kDistBase[dsym] + extra;
            if (distance > o.n) return fail("distance too far back");
            if (o.n + length <= o.cap) {
                uint8_t *d = o.out + o.n;
                const uint8_t *s = d - distance;
                for (size_t i = 0; i < length; ++i) d[i] = s[i]; // (forward, byte by byte: an overlapping match repeats)
                o.n += length;
            } else
                for (size_t i = 0; i < length; ++i) o.put(o.at(o.n - distance));
        }
    }
    bool dynamic() // inflate_dynamic (:386-458)
    {
        uint32_t hlit, hdist, hclen, v;
        if (!r.read(5, &hlit) || !r.read(5, &hdist) || !r.read(4, &hclen)) return fail(kEnd);
        hlit += 257; hdist += 1; hclen += 4;
        uint8_t cl[19] = {};
        for (uint32_t i = 0; i < hclen; ++i) {
            if (!r.read(3, &v)) return fail(kEnd);
            cl[kCodeLengthOrder[i]] = static_cast<uint8_t>(v);
        }
        Huff clt;
        clt.build(cl, 19);
        uint8_t lengths[288 + 32] = {};
        const uint32_t total = hlit + hdist;
        const char *e = nullptr;
        for (uint32_t i = 0; i < total;) {
            uint32_t sym;
            if (!clt.decode(r, &sym, &e)) return fail(e);
            if (sym < 16) { lengths[i++] = static_cast<uint8_t>(sym); continue; }
            uint32_t repeat;
            uint8_t value = 0;
            if (sym == 16) {
                if (i == 0) return fail("repeat code at start");
                if (!r.read(2, &repeat)) return fail(kEnd);
                repeat += 3;
                value = lengths[i - 1];
            } else if (sym == 17) {
                if (!r.read(3, &repeat)) return fail(kEnd);
                repeat += 3;
            } else {
                if (!r.read(7, &repeat)) return fail(kEnd);
                repeat += 11;
            }
            for (uint32_t k = 0; k < repeat; ++k) {
                if (i >= total) return fail("too many code lengths");
                lengths[i++] = value;
            }
        }
        Huff lit, dist;
        lit.build(lengths, hlit);
        dist.build(lengths + hlit, hdist);
        return block(lit, dist);
    }
    bool run() // inflate_with_size (:265-287)
    {
        static const FixedTables fixed;
        for (;;) {
            uint32_t bfinal, btype;
            if (!r.read(1, &bfinal) || !r.read(2, &btype)) return fail(kEnd);
            const bool ok = btype == 0 ? stored() : btype == 1 ? block(fixed.lit, fixed.dist) : btype == 2 ? dynamic() : fail("reserved block type");
            if (!ok) return false;
            if (bfinal) return true;
        }
    }
};

std::string hex8(uint32_t v)
{
    char b[9];
    static const char d[] = "0123456789ABCDEF";
    for (int i = 0; i < 8; ++i) b[i] = d[(v >> (28 - 4 * i)) & 15];
    b[8] = 0;
    return b;
}

} // namespace

uint32_t adler32(const uint8_t *data, size_t len, uint32_t start)
{
    uint32_t a = start & 0xFFFFu, b = start >> 16;
    while (len) {
        const size_t run = len < 5552 ? len : 5552; // the longest run whose sums cannot overflow 32 bits
        for (size_t i = 0; i < run; ++i) { a += data[i]; b += a; }
        a %= 65521u; b %= 65521u;
        data += run; len -= run;
    }
    return (b << 16) | a;
}

Kind inflate_zlib(const uint8_t *data, size_t len, uint8_t *out, size_t expected, std::string *msg)
{
    if (len < 6) { *msg = "zlib stream too short"; return INVALID; }
    const uint8_t cmf = data[0], flg = data[1];
    if ((cmf & 0x0F) != 8) { *msg = "invalid zlib compression method"; return INVALID; }
    if (((static_cast<unsigned>(cmf) << 8) | flg) % 31 != 0) { *msg = "invalid zlib header checksum"; return INVALID; }
    if (flg & 0x20) { *msg = "preset dictionary not supported"; return UNSUPPORTED; }
    const size_t end = len - 4;
    Sink *sink = new Sink(out, expected); // (the ring: 32 KiB, not on the stack)
    Inflater inf(data + 2, end - 2, *sink);
    Kind kind = OK;
    if (!inf.run()) { *msg = inf.err; kind = INVALID; }
    else {
        const uint32_t stored = (static_cast<uint32_t>(data[end]) << 24) | (static_cast<uint32_t>(data[end + 1]) << 16) |
                                (static_cast<uint32_t>(data[end + 2]) << 8) | data[end + 3];
        const uint32_t computed = sink->adler();
        if (stored != computed) { *msg = "Adler32 mismatch: expected " + hex8(stored) + ", got " + hex8(computed); kind = INVALID; }
        else if (sink->n != expected) {
            *msg = "decompressed size mismatch: expected " + std::to_string(expected) + ", got " + std::to_string(sink->n);
            kind = INVALID;
        }
    }
    delete sink;
    return kind;
}

} // namespace pixo_inflate
