// png_inflate_math.h — the device inflate of the PNG decode batches (png_inflate.hip), written so that it also compiles
// for the host (tests/emu_png_inflate/): one zlib-wrapped DEFLATE stream (RFC 1950 / 1951) decoded by ONE wavefront.
//
// The walk has two kinds of code.  UNIFORM code — the bit buffer, the table lookups, the forming of tokens — computes the
// same values on every lane; what it reads from LDS goes through PNGI_UNI (v_readfirstlane), so the compiler can keep it
// on the scalar side.  LANE code stands in PNGI_LANES(lane) { ... } regions: on the device every lane runs the body once
// between two workgroup barriers (the workgroup IS the wavefront), on the host the body runs for lane 0..63 in turn.  Both
// give the same bytes because of the one rule every region keeps: no lane reads a location another lane writes in the same
// region.  (Uniform code that stores to LDS stores the same value from every lane.)
//
//   tokens  A literal or a match, kept in LDS with the output position it starts at — the uniform decode has that position
//           anyway (it checks every distance against it), so no prefix sum over the lengths is needed.  A step is at most
//           kStepTokens tokens: all lanes store the step's literals, then the matches are copied in token order, each by all
//           lanes; a match shorter than its length repeats: byte i comes from src[i % distance].
//   ring    The last kWindowBytes of output live in an LDS ring, flushed to global memory in 16-byte pieces; matches never
//           read global memory.  The ring is exactly the window, so a store at position p destroys position p - 32768:
//           harmless in token order, but a step stores its literals FIRST.  A literal behind a match in the same step can
//           only hit that match's source if the match reaches further back than kWindowBytes - kStepMaxBytes: such a match
//           (kFarDistance) closes its step.
//   adler   accumulated at the flush: per-lane sums over 16-byte pieces, combined modulo 65521 by uniform code.
//   tables  canonical: per code length the first code, the count and the offset into the symbols sorted by (length, symbol),
//           and a 2^kLutBits-entry lookup for codes of up to kLutBits bits, all built by the lanes together.  A set whose
//           Kraft sum exceeds 1 is not decoded (NEEDS_HOST); complete and incomplete sets are, an unused code is FAILED.
//
// Termination: every turn of a loop in the walk consumes at least one input bit or produces at least one output byte (a
// stored block of length 0 consumes its 3 header bits), and the walk stops with FAILED when either runs out.  So a stream
// of in_len bytes asked for `expected` bytes takes at most 8 * in_len + expected + 1 turns, all loops of the walk together
// (Walk::turns counts them; the table builds inside a turn are bounded by the code sizes).
// Bounds: reads in[0, 4 * ceil(in_len / 4)) as aligned dwords — `in` is 4-byte aligned and padded —, writes out[0, n) for the
// n <= expected bytes it produced, 16 bytes at a time only where the address is 16-byte aligned and all 16 lie below n.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PNGI_HD __host__ __device__ __forceinline__
#else
#define PNGI_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PNGI_UNI(x) static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x)))
#define PNGI_LANES(lane) for (uint32_t lane = (__syncthreads(), threadIdx.x), once_ = 1; once_; once_ = 0, __syncthreads())
#define PNGI_TURN() ((void)0)
#else
#define PNGI_TURN() (++turns)
#define PNGI_UNI(x) static_cast<uint32_t>(x)
#define PNGI_LANES(lane) for (uint32_t lane = 0; lane < ::pixo_pngi::kLanes; ++lane)
#endif

namespace pixo_pngi {

constexpr uint32_t kLanes = 64;
constexpr uint32_t kStepTokens = 64;                              // tokens a step holds at most
constexpr uint32_t kWindowBytes = 32768;                          // the ring: exactly DEFLATE's window
constexpr uint32_t kMaxMatch = 258;
constexpr uint32_t kStepMaxBytes = kStepTokens * kMaxMatch;       // 16512: what a step produces at most
constexpr uint32_t kFarDistance = kWindowBytes - kStepMaxBytes;   // 16256: a match further back than this closes its step
constexpr uint32_t kStoredChunk = 4096;                           // bytes of a stored block copied between two flush checks
constexpr uint32_t kFlushPiece = 16;
constexpr uint32_t kLutBits = 10;
constexpr uint32_t kMaxBits = 15;
constexpr uint32_t kAdlerMod = 65521;
static_assert(kStepTokens == kLanes, "a token per lane");
static_assert(kStepMaxBytes + kFlushPiece <= kWindowBytes && kStoredChunk + kFlushPiece <= kWindowBytes, "a flush makes room for a step");

enum Verdict : uint32_t { OK = 0, FAILED = 1, NEEDS_HOST = 2 };

// One code set.  `lut` entries: symbol | length << 12, 0: no code of up to kLutBits bits starts like this.
struct Huff {
    uint16_t lut[1u << kLutBits];
    uint16_t count[kMaxBits + 1], first[kMaxBits + 1], offset[kMaxBits + 1];
    uint16_t sorted[288];
};
// What the wavefront keeps in LDS
struct Shared {
    alignas(16) uint8_t ring[kWindowBytes];
    Huff lit, dist; // (the code-length code is built in `dist`, which is not needed before the lengths are read)
    uint8_t lengths[320];
    uint32_t tok[kStepTokens][2]; // [0]: length | (distance - 1) << 9 | literal << 24 (length 1: a literal), [1]: the position, low 32 bits
    uint32_t sum_a[kLanes], sum_b[kLanes];
};

PNGI_HD uint32_t length_base(uint32_t c, uint32_t *extra) // c = symbol - 257, 0..28
{
    if (c < 8) { *extra = 0; return c + 3; }
    if (c == 28) { *extra = 0; return 258; }
    const uint32_t e = (c >> 2) - 1;
    *extra = e;
    return ((4 + (c & 3)) << e) + 3;
}
PNGI_HD uint32_t distance_base(uint32_t d, uint32_t *extra) // d = 0..29
{
    if (d < 4) { *extra = 0; return d + 1; }
    const uint32_t e = (d >> 1) - 1;
    *extra = e;
    return ((2 + (d & 1)) << e) + 1;
}
PNGI_HD uint32_t fixed_length(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : s < 288 ? 8u : 5u; } // 288..319: the distances

// Kraft sum of the counts in units of 2^-15: above 2^15 the set is over-subscribed
PNGI_HD uint32_t kraft_units(const uint32_t count[kMaxBits + 1])
{
    uint32_t k = 0;
    for (uint32_t l = 1; l <= kMaxBits; ++l) k += count[l] << (kMaxBits - l);
    return k;
}
// The symbol whose code the low bits of `bits` start with (first bit of the code lowest), among the codes of at most
// `max_len` bits: symbol | length << 12, or 0.  (Canonical codes, RFC 1951 3.2.2.)
PNGI_HD uint32_t canonical_entry(const Huff &h, uint32_t bits, uint32_t max_len)
{
    uint32_t code = 0;
    for (uint32_t l = 1; l <= max_len; ++l) {
        code = (code << 1) | ((bits >> (l - 1)) & 1);
        const uint32_t first = h.first[l], d = code - first;
        if (code >= first && d < h.count[l]) return h.sorted[h.offset[l] + d] | (l << 12);
    }
    return 0;
}
// Where byte i of a match comes from, relative to the match's first source byte (position - distance)
PNGI_HD uint32_t match_source(uint32_t i, uint32_t distance) { return distance < kLanes ? (distance == 1 ? 0u : i % distance) : i; }

PNGI_HD uint32_t token_literal(uint32_t byte) { return 1u | (byte << 24); }
PNGI_HD uint32_t token_match(uint32_t length, uint32_t distance) { return length | ((distance - 1) << 9); }
PNGI_HD uint32_t token_length(uint32_t t) { return t & 511u; }
PNGI_HD uint32_t token_distance(uint32_t t) { return ((t >> 9) & 32767u) + 1; }

struct Result {
    uint32_t verdict, adler;
    uint64_t produced;
};

// The walk over one stream.  `sh`: the wavefront's LDS (host: any memory).
struct Walk {
    Shared &sh;
    const uint32_t *in; // the stream's DEFLATE bytes (behind the 2-byte zlib header), as aligned dwords
    uint64_t in_dwords, in_bits;
    uint8_t *out;
    uint64_t expected;
    bool out_aligned;
    // the bit buffer: `cnt` valid bits in `buf`, the next dword to load, bits consumed so far
    uint64_t buf = 0, next = 0, used = 0;
    uint32_t cnt = 0;
    // the output: n bytes decoded (tokens included), `done` of them in the ring, `flushed` in global memory
    uint64_t n = 0, done = 0, flushed = 0;
    uint32_t adler_a = 1, adler_b = 0;
    uint32_t ntok = 0;
    uint64_t match_mask = 0; // which tokens of the step are matches
    bool fixed_held = false; // sh.lit / sh.dist hold the fixed code
    uint64_t turns = 0;      // (the bound above; counted by host builds only, which check it)

    PNGI_HD Walk(Shared &s, const uint8_t *in_bytes, uint64_t in_len, uint8_t *o, uint64_t exp)
        : sh(s), in(reinterpret_cast<const uint32_t *>(in_bytes)), in_dwords((in_len + 3) / 4), in_bits(in_len * 8), out(o), expected(exp),
          out_aligned(reinterpret_cast<uintptr_t>(o) % kFlushPiece == 0)
    {
    }

    // ---- bits (uniform) -------------------------------------------------------------------------------------------------
    PNGI_HD void refill() // afterwards cnt > 32
    {
        if (cnt <= 32) {
            const uint64_t w = next < in_dwords ? in[next] : 0u;
            buf |= w << cnt;
            cnt += 32;
            ++next;
        }
    }
    PNGI_HD bool have(uint32_t k) const { return used + k <= in_bits; }
    PNGI_HD void consume(uint32_t k) { buf >>= k; cnt -= k; used += k; }
    PNGI_HD bool read(uint32_t k, uint32_t *v) // k <= 16
    {
        refill();
        if (!have(k)) return false;
        *v = static_cast<uint32_t>(buf) & ((1u << k) - 1);
        consume(k);
        return true;
    }
    PNGI_HD void seek(uint64_t bit) // the bit buffer starts over at this bit of the stream
    {
        buf = 0; cnt = 0; next = bit / 32; used = bit & ~uint64_t{31};
        refill();
        consume(static_cast<uint32_t>(bit & 31));
    }
    // One symbol of `h`; false: the code is unused, or the input ends inside it
    PNGI_HD bool decode(const Huff &h, uint32_t *symbol)
    {
        refill();
        const uint32_t bits = static_cast<uint32_t>(buf) & ((1u << kMaxBits) - 1);
        uint32_t e = PNGI_UNI(h.lut[bits & ((1u << kLutBits) - 1)]);
        if (!e) { // a code longer than the lookup, or none
            uint32_t code = 0;
            for (uint32_t l = 1; l <= kMaxBits && !e; ++l) {
                code = (code << 1) | ((bits >> (l - 1)) & 1);
                const uint32_t first = PNGI_UNI(h.first[l]), d = code - first;
                if (code >= first && d < PNGI_UNI(h.count[l])) e = PNGI_UNI(h.sorted[PNGI_UNI(h.offset[l]) + d]) | (l << 12);
            }
            if (!e) return false;
        }
        const uint32_t len = e >> 12;
        if (!have(len)) return false;
        consume(len);
        *symbol = e & 0xFFFu;
        return true;
    }

    // ---- tables (lanes together) ------------------------------------------------------------------------------------------
    // sh.lengths[from, from + symbols) -> h.  False: over-subscribed.
    PNGI_HD bool build(Huff &h, uint32_t from, uint32_t symbols)
    {
        PNGI_LANES(lane) {
            if (lane > kMaxBits) continue;
            uint32_t c = 0;
            for (uint32_t s = 0; s < symbols; ++s) c += sh.lengths[from + s] == lane;
            h.count[lane] = static_cast<uint16_t>(lane ? c : 0);
        }
        uint32_t count[kMaxBits + 1];
        for (uint32_t l = 0; l <= kMaxBits; ++l) count[l] = PNGI_UNI(h.count[l]);
        if (kraft_units(count) > (1u << kMaxBits)) return false;
        uint32_t code = 0, at = 0;
        for (uint32_t l = 1; l <= kMaxBits; ++l) { // (Kraft <= 1: every first code fits its length)
            code = (code + count[l - 1]) << 1;
            h.first[l] = static_cast<uint16_t>(code);
            h.offset[l] = static_cast<uint16_t>(at);
            at += count[l];
        }
        PNGI_LANES(lane) {
            if (lane == 0 || lane > kMaxBits) continue;
            uint32_t k = h.offset[lane];
            for (uint32_t s = 0; s < symbols; ++s)
                if (sh.lengths[from + s] == lane) h.sorted[k++] = static_cast<uint16_t>(s);
        }
        PNGI_LANES(lane) {
            for (uint32_t j = lane; j < (1u << kLutBits); j += kLanes) h.lut[j] = static_cast<uint16_t>(canonical_entry(h, j, kLutBits));
        }
        return true;
    }

    // ---- output -------------------------------------------------------------------------------------------------------------
    // ring[flushed, upto) -> out, and into the Adler-32.  upto <= done; a multiple of 16 from `flushed` on unless it is the end.
    PNGI_HD void flush(uint64_t upto)
    {
        const uint32_t len = static_cast<uint32_t>(upto - flushed); // <= kWindowBytes
        if (!len) return;
        const uint32_t at = static_cast<uint32_t>(flushed) & (kWindowBytes - 1); // (a multiple of 16)
        uint8_t *dst = out + flushed;
        PNGI_LANES(lane) {
            uint32_t a = 0;
            uint64_t b = 0;
            for (uint32_t off = lane * kFlushPiece; off < len; off += kLanes * kFlushPiece) {
                const uint32_t valid = len - off < kFlushPiece ? len - off : kFlushPiece;
                const uint8_t *src = sh.ring + ((at + off) & (kWindowBytes - 1));
                uint32_t w[4];
                memcpy(w, __builtin_assume_aligned(src, 16), sizeof w);
                uint32_t s = 0, t = 0; // the piece's sum, and its sum weighted by the index in the piece
#pragma unroll
                for (uint32_t k = 0; k < kFlushPiece; ++k) { // (constant indices: the piece stays in registers)
                    const uint32_t v = k < valid ? (w[k >> 2] >> (8 * (k & 3))) & 255u : 0u;
                    s += v;
                    t += k * v;
                }
                a += s;
                b += static_cast<uint64_t>(len - off) * s - t; // byte k of the flush counts len - k times in b
                if (valid == kFlushPiece && out_aligned) memcpy(__builtin_assume_aligned(dst + off, 16), w, sizeof w);
                else {
#pragma unroll
                    for (uint32_t k = 0; k < kFlushPiece; ++k)
                        if (k < valid) dst[off + k] = static_cast<uint8_t>(w[k >> 2] >> (8 * (k & 3)));
                }
            }
            sh.sum_a[lane] = a;
            sh.sum_b[lane] = static_cast<uint32_t>(b % kAdlerMod);
        }
        uint64_t a = 0, b = 0;
        for (uint32_t l = 0; l < kLanes; ++l) { a += PNGI_UNI(sh.sum_a[l]); b += PNGI_UNI(sh.sum_b[l]); }
        b += static_cast<uint64_t>(len) * adler_a + adler_b;
        adler_a = static_cast<uint32_t>((adler_a + a) % kAdlerMod);
        adler_b = static_cast<uint32_t>(b % kAdlerMod);
        flushed = upto;
    }
    // Room in the ring for output up to position `end`: what is not in global memory yet must not be overwritten
    PNGI_HD void make_room(uint64_t end)
    {
        if (end - flushed > kWindowBytes) flush(done & ~uint64_t{kFlushPiece - 1});
    }
    // The pending tokens into the ring
    PNGI_HD void run_step()
    {
        if (!ntok) return;
        make_room(n);
        const uint32_t count = ntok;
        PNGI_LANES(lane) {
            if (lane >= count) continue;
            const uint32_t t = sh.tok[lane][0];
            if (token_length(t) == 1) sh.ring[sh.tok[lane][1] & (kWindowBytes - 1)] = static_cast<uint8_t>(t >> 24);
        }
        for (uint64_t m = match_mask; m; m &= m - 1) {
            const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(m));
            const uint32_t t = PNGI_UNI(sh.tok[k][0]), p = PNGI_UNI(sh.tok[k][1]);
            const uint32_t len = token_length(t), dist = token_distance(t);
            if (dist < kLanes) { // every source byte lies in front of the match: one region
                PNGI_LANES(lane) {
                    for (uint32_t i = lane; i < len; i += kLanes)
                        sh.ring[(p + i) & (kWindowBytes - 1)] = sh.ring[(p - dist + match_source(i, dist)) & (kWindowBytes - 1)];
                }
            } else // 64 bytes a region: a region's sources were stored by the regions before it
                for (uint32_t base = 0; base < len; base += kLanes) {
                    PNGI_LANES(lane) {
                        const uint32_t i = base + lane;
                        if (i < len) sh.ring[(p + i) & (kWindowBytes - 1)] = sh.ring[(p - dist + i) & (kWindowBytes - 1)];
                    }
                }
        }
        done = n;
        ntok = 0;
        match_mask = 0;
    }

    // ---- blocks -------------------------------------------------------------------------------------------------------------
    // (between blocks no token is pending: huffman_block runs its last step before it returns)
    PNGI_HD uint32_t stored()
    {
        refill();
        consume(static_cast<uint32_t>((8 - (used & 7)) & 7)); // (the rest of the byte the header ended in)
        uint32_t len, nlen;
        if (!read(16, &len) || !read(16, &nlen)) return FAILED;
        if (len != ((~nlen) & 0xFFFFu)) return FAILED;
        if (!have(8 * len)) return FAILED;
        if (len > expected - n) return FAILED;
        const uint8_t *src = reinterpret_cast<const uint8_t *>(in) + used / 8;
        for (uint32_t at = 0; at < len; at += kStoredChunk) {
            PNGI_TURN();
            const uint32_t chunk = len - at < kStoredChunk ? len - at : kStoredChunk;
            make_room(n + chunk);
            const uint32_t p = static_cast<uint32_t>(n);
            PNGI_LANES(lane) {
                for (uint32_t i = lane; i < chunk; i += kLanes) sh.ring[(p + i) & (kWindowBytes - 1)] = src[at + i];
            }
            n += chunk;
            done = n;
        }
        seek(used + 8 * static_cast<uint64_t>(len));
        return OK;
    }
    // One token of the block into *token / *length: OK, or why the block ends here (kEndOfBlock: as it should)
    static constexpr uint32_t kEndOfBlock = 3;
    PNGI_HD uint32_t next_token(uint32_t *token, uint32_t *length, bool *far)
    {
        uint32_t sym, extra, bits;
        if (!decode(sh.lit, &sym)) return FAILED;
        if (sym < 256) {
            if (n >= expected) return FAILED;
            *token = token_literal(sym); *length = 1; *far = false;
            return OK;
        }
        if (sym == 256) return kEndOfBlock;
        if (sym > 285) return FAILED;
        uint32_t len = length_base(sym - 257, &extra);
        if (!read(extra, &bits)) return FAILED;
        len += bits;
        if (!decode(sh.dist, &sym) || sym >= 30) return FAILED;
        uint32_t distance = distance_base(sym, &extra);
        if (!read(extra, &bits)) return FAILED;
        distance += bits;
        if (distance > n || len > expected - n) return FAILED;
        *token = token_match(len, distance); *length = len; *far = distance > kFarDistance;
        return OK;
    }
    PNGI_HD uint32_t huffman_block()
    {
        for (;;) {
            PNGI_TURN();
            uint32_t token = 0, length = 0;
            bool far = false;
            const uint32_t what = next_token(&token, &length, &far);
            if (what == OK) {
                sh.tok[ntok][0] = token;
                sh.tok[ntok][1] = static_cast<uint32_t>(n);
                if (length > 1) match_mask |= uint64_t{1} << ntok;
                ++ntok;
                n += length;
            }
            if (what != OK || far || ntok == kStepTokens) run_step(); // (a failing block's tokens so far were sound: they are run too)
            if (what != OK) return what == kEndOfBlock ? static_cast<uint32_t>(OK) : what;
        }
    }
    PNGI_HD static uint32_t code_length_order(uint32_t i) // RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
    {
        constexpr uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                                11ull << 50 | 4ull << 55;
        constexpr uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
        return static_cast<uint32_t>((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
    }
    // The lengths of a dynamic block's two codes into sh.lengths: literal/length code first, then the distance code
    PNGI_HD uint32_t dynamic_lengths(uint32_t *hlit, uint32_t *hdist)
    {
        uint32_t hclen, v;
        if (!read(5, hlit) || !read(5, hdist) || !read(4, &hclen)) return FAILED;
        *hlit += 257; *hdist += 1; hclen += 4;
        PNGI_LANES(lane) {
            if (lane < 19) sh.lengths[lane] = 0;
        }
        for (uint32_t i = 0; i < hclen; ++i) {
            if (!read(3, &v)) return FAILED;
            sh.lengths[code_length_order(i)] = static_cast<uint8_t>(v);
        }
        if (!build(sh.dist, 0, 19)) return NEEDS_HOST;
        const uint32_t total = *hlit + *hdist;
        uint32_t prev = 0;
        for (uint32_t i = 0; i < total;) {
            PNGI_TURN();
            uint32_t sym, repeat, value = 0;
            if (!decode(sh.dist, &sym)) return FAILED;
            if (sym < 16) { sh.lengths[i++] = static_cast<uint8_t>(sym); prev = sym; continue; }
            if (sym == 16) {
                if (i == 0 || !read(2, &repeat)) return FAILED;
                repeat += 3;
                value = prev;
            } else if (sym == 17) {
                if (!read(3, &repeat)) return FAILED;
                repeat += 3;
            } else {
                if (!read(7, &repeat)) return FAILED;
                repeat += 11;
            }
            if (repeat > total - i) return FAILED;
            for (uint32_t k = 0; k < repeat; ++k) sh.lengths[i++] = static_cast<uint8_t>(value);
            prev = value;
        }
        return OK;
    }
    PNGI_HD uint32_t coded_block(bool dynamic)
    {
        uint32_t hlit = 288, hdist = 32;
        if (dynamic) {
            fixed_held = false;
            const uint32_t rc = dynamic_lengths(&hlit, &hdist);
            if (rc != OK) return rc;
        } else if (!fixed_held) {
            PNGI_LANES(lane) {
                for (uint32_t s = lane; s < 320; s += kLanes) sh.lengths[s] = static_cast<uint8_t>(fixed_length(s));
            }
        }
        if (dynamic || !fixed_held) {
            bool sound = true;
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
            for (uint32_t t = 0; t < 2; ++t) sound = build(t ? sh.dist : sh.lit, t ? hlit : 0, t ? hdist : hlit) && sound;
            if (!sound) return NEEDS_HOST;
            fixed_held = !dynamic;
        }
        return huffman_block();
    }

    PNGI_HD Result run()
    {
        uint32_t verdict;
        for (;;) {
            PNGI_TURN();
            uint32_t bfinal, btype;
            if (!read(1, &bfinal) || !read(2, &btype)) { verdict = FAILED; break; }
            verdict = btype == 0 ? stored() : btype == 3 ? static_cast<uint32_t>(FAILED) : coded_block(btype == 2);
            if (verdict != OK) break;
            if (bfinal) { verdict = n == expected ? OK : FAILED; break; }
        }
        // whatever was decoded reaches global memory: `produced` bytes of the region and their Adler-32 are valid for every verdict
        flush(done); // (at most kWindowBytes are ever left: make_room)
        Result r;
        r.verdict = verdict;
        r.adler = (adler_b << 16) | adler_a;
        r.produced = done;
        return r;
    }
};

// Host-side helper of the driver and the tests: Adler-32 as the walk accumulates it
PNGI_HD uint32_t adler32_bytes(const uint8_t *p, uint64_t len)
{
    uint64_t a = 1, b = 0;
    for (uint64_t i = 0; i < len; ++i) { a = (a + p[i]) % kAdlerMod; b = (b + a) % kAdlerMod; }
    return static_cast<uint32_t>((b << 16) | a);
}

} // namespace pixo_pngi
