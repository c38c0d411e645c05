// png_deflate_math.h — the arithmetic of the device DEFLATE (png_deflate.hip), written so that it also compiles for the
// host (tests/emu_png_deflate/): symbol mapping of RFC 1951, the length-limited Huffman code lengths, canonical codes for the
// LSB-first writer, the dynamic block header with its 16/17/18 run codes, the bit writer, and the CRC-32 combine the host
// uses to join the device's piece values.  Everything here is single-threaded: the kernel runs it on one lane per tree.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PNGZ_HD __host__ __device__ inline
#else
#define PNGZ_HD inline
#endif

namespace pixo_pngz {

constexpr uint32_t kLitSyms = 286, kDistSyms = 30, kClSyms = 19;
constexpr uint32_t kLitTable = 288, kDistTable = 32; // the fixed code assigns codes to 288 / 32 symbols
constexpr uint32_t kMinMatch = 3, kMaxMatch = 258, kWindow = 32768;
constexpr uint32_t kHeaderBytes = 704; // > 17 + 19 * 3 + 316 * 14 bits

// A token: len << 16 | dist for a match (len 3..258, dist 1..32768), the byte itself for a literal (len field 0).
PNGZ_HD uint32_t token_match(uint32_t len, uint32_t dist) { return (len << 16) | dist; }
PNGZ_HD uint32_t token_len(uint32_t t) { return t >> 16; }

PNGZ_HD uint32_t floor_log2(uint32_t v) { return 31u - static_cast<uint32_t>(__builtin_clz(v)); } // v > 0

// length 3..258 -> symbol 257..285, its extra bits and their value
PNGZ_HD void length_symbol(uint32_t len, uint32_t *sym, uint32_t *ebits, uint32_t *evalue)
{
    const uint32_t l = len - 3;
    if (len == 258) { *sym = 285; *ebits = 0; *evalue = 0; return; }
    if (l < 8) { *sym = 257 + l; *ebits = 0; *evalue = 0; return; }
    const uint32_t e = floor_log2(l) - 2;
    *sym = 261 + 4 * e + ((l >> e) - 4);
    *ebits = e;
    *evalue = l & ((1u << e) - 1);
}
// distance 1..32768 -> symbol 0..29
PNGZ_HD void distance_symbol(uint32_t dist, uint32_t *sym, uint32_t *ebits, uint32_t *evalue)
{
    const uint32_t d = dist - 1;
    if (d < 4) { *sym = d; *ebits = 0; *evalue = 0; return; }
    const uint32_t e = floor_log2(d) - 1;
    *sym = 2 * e + 2 + ((d >> e) & 1);
    *ebits = e;
    *evalue = d & ((1u << e) - 1);
}
PNGZ_HD uint32_t length_symbol_extra(uint32_t sym) { return sym < 265 || sym == 285 ? 0u : (sym - 261) >> 2; } // sym 257..285
PNGZ_HD uint32_t distance_symbol_extra(uint32_t sym) { return sym < 4 ? 0u : (sym >> 1) - 1; }
PNGZ_HD uint32_t fixed_literal_length(uint32_t sym) { return sym < 144 ? 8u : sym < 256 ? 9u : sym < 280 ? 7u : 8u; }

// ---- the high-effort finder: links, chains, the lazy rule --------------------------------------------
// Positions are counted from the start of the chunk's window.  A link is the distance from a position to the head its
// look-up saw (head: position + 1 of the latest occurrence of the hash in earlier sub-steps, 0: none); 0 ends the chain.
// A distance beyond the window is not kept: every later entry of the chain lies farther still.
PNGZ_HD uint32_t chain_link(uint32_t pos, uint32_t head)
{
    if (!head) return 0;
    const uint32_t d = pos + 1 - head; // head <= pos: inserted by an earlier sub-step
    return d > kWindow ? 0 : d;
}
// The next entry of the chain of a position: `dist` is the distance of the entry the link was read at (0: the
// position itself), `link` that entry's link.  -> the new entry's distance, 0: the chain ends here.
PNGZ_HD uint32_t chain_step(uint32_t dist, uint32_t link)
{
    if (!link || dist + link > kWindow) return 0;
    return dist + link;
}
// What a finder keeps of the best match at a position: nothing below 3 bytes, and no 3 bytes from beyond 4096.
PNGZ_HD uint32_t kept_length(uint32_t len, uint32_t dist) { return len < kMinMatch || (len == kMinMatch && dist > 4096) ? 0 : len; }
// One-step lazy parse: the position is given up as a literal when the next one has a strictly longer match
// (len_next: 0 where there is none, or no next position in the chunk).
PNGZ_HD bool lazy_defers(uint32_t len_here, uint32_t len_next) { return len_next > len_here; }
PNGZ_HD uint32_t lazy_next(uint32_t p, uint32_t len_here, uint32_t len_next)
{
    return lazy_defers(len_here, len_next) ? p + 1 : p + (len_here ? len_here : 1);
}

// ---- LSB-first bit writer over bytes ---------------------------------------------------------------------------------
struct BitWriter {
    uint8_t *p;
    uint32_t pos = 0, n = 0;
    uint64_t acc = 0;
    PNGZ_HD explicit BitWriter(uint8_t *dst) : p(dst) {}
    PNGZ_HD void put(uint32_t value, uint32_t bits) // bits <= 32
    {
        acc |= static_cast<uint64_t>(value) << n;
        n += bits;
        while (n >= 8) { p[pos++] = static_cast<uint8_t>(acc); acc >>= 8; n -= 8; }
    }
    PNGZ_HD uint32_t bit_count() const { return pos * 8 + n; }
    PNGZ_HD void flush() { if (n) { p[pos++] = static_cast<uint8_t>(acc); acc = 0; n = 0; } } // pads with zero bits
};

// ---- code lengths ------------------------------------------------------------------------------------------------------
// Scratch of one tree (the kernel keeps it in LDS).
struct HuffWork {
    uint32_t key[2][kLitTable];
    uint16_t sym[2][kLitTable];
    uint16_t bucket[256];
    uint16_t per_length[33];
    uint16_t runs[kLitSyms + kDistSyms + 4]; // header coder: code-length symbols, extra value << 8
};

// Lengths of a Huffman code for freq[0..n), none above max_bits (max_bits <= 15), symbols of frequency 0 get length 0.
// The code is complete (Kraft sum exactly 1): an alphabet with fewer than two symbols in use is filled up with symbol
// 0 and / or 1 at length 1, as zlib does, so that no decoder meets an incomplete code.  n >= 2.
// Method: sort by frequency (LSD radix), the in-place minimum-redundancy lengths of Moffat and Katajainen, then the
// overflow of lengths above max_bits is paid for by lengthening the shortest codes that can spare it.
PNGZ_HD void huffman_lengths(const uint32_t *freq, uint32_t n, uint32_t max_bits, uint8_t *lens, HuffWork &w)
{
    uint32_t used = 0;
    for (uint32_t i = 0; i < n; ++i) {
        lens[i] = 0;
        if (freq[i]) { w.key[0][used] = freq[i]; w.sym[0][used] = static_cast<uint16_t>(i); ++used; }
    }
    if (used < 2) {
        const uint32_t only = used ? w.sym[0][0] : 0;
        lens[only] = 1;
        lens[only == 0 ? 1 : 0] = 1;
        return;
    }
    int cur = 0;
    for (uint32_t shift = 0; shift < 32; shift += 8) { // stable: equal frequencies stay in symbol order
        uint32_t top = 0;
        for (uint32_t i = 0; i < used; ++i) top |= w.key[cur][i] >> shift;
        if (!top) break;
        for (uint32_t b = 0; b < 256; ++b) w.bucket[b] = 0;
        for (uint32_t i = 0; i < used; ++i) ++w.bucket[(w.key[cur][i] >> shift) & 255];
        uint32_t at = 0;
        for (uint32_t b = 0; b < 256; ++b) { const uint32_t c = w.bucket[b]; w.bucket[b] = static_cast<uint16_t>(at); at += c; }
        for (uint32_t i = 0; i < used; ++i) {
            const uint32_t d = w.bucket[(w.key[cur][i] >> shift) & 255]++;
            w.key[cur ^ 1][d] = w.key[cur][i];
            w.sym[cur ^ 1][d] = w.sym[cur][i];
        }
        cur ^= 1;
    }
    uint32_t *a = w.key[cur];
    const int m = static_cast<int>(used);
    { // Moffat-Katajainen: a[] ascending frequencies in, a[] code lengths out (longest first)
        a[0] += a[1];
        int root = 0, leaf = 2, next;
        for (next = 1; next < m - 1; ++next) {
            if (leaf >= m || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = static_cast<uint32_t>(next); }
            else a[next] = a[leaf++];
            if (leaf >= m || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = static_cast<uint32_t>(next); }
            else a[next] += a[leaf++];
        }
        a[m - 2] = 0;
        for (next = m - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
        int avail = 1, inner = 0;
        uint32_t depth = 0;
        root = m - 2;
        next = m - 1;
        while (avail > 0) {
            while (root >= 0 && a[root] == depth) { ++inner; --root; }
            while (avail > inner) { a[next--] = depth; --avail; }
            avail = 2 * inner;
            ++depth;
            inner = 0;
        }
    }
    for (uint32_t i = 0; i <= 32; ++i) w.per_length[i] = 0;
    for (int i = 0; i < m; ++i) ++w.per_length[a[i] < max_bits ? a[i] : max_bits];
    uint32_t total = 0;
    for (uint32_t i = max_bits; i > 0; --i) total += static_cast<uint32_t>(w.per_length[i]) << (max_bits - i);
    while (total != (1u << max_bits)) { // only ever above: clamping can only raise the Kraft sum
        --w.per_length[max_bits];
        for (uint32_t i = max_bits - 1; i > 0; --i)
            if (w.per_length[i]) { --w.per_length[i]; w.per_length[i + 1] += 2; break; }
        --total;
    }
    int j = m;
    for (uint32_t l = 1; l <= max_bits; ++l)
        for (uint32_t k = w.per_length[l]; k > 0; --k) lens[w.sym[cur][--j]] = static_cast<uint8_t>(l);
}

PNGZ_HD uint32_t reverse_bits(uint32_t v, uint32_t bits)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < bits; ++i) { r = (r << 1) | (v & 1); v >>= 1; }
    return r;
}
// Canonical codes of RFC 1951 §3.2.2 for lens[0..n), each reversed so that it is written LSB first.
PNGZ_HD void canonical_codes(const uint8_t *lens, uint32_t n, uint16_t *codes)
{
    uint32_t count[16], next[16];
    for (uint32_t i = 0; i < 16; ++i) count[i] = 0;
    for (uint32_t i = 0; i < n; ++i) ++count[lens[i]];
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (uint32_t b = 1; b < 16; ++b) { code = (code + count[b - 1]) << 1; next[b] = code; }
    for (uint32_t i = 0; i < n; ++i) codes[i] = lens[i] ? static_cast<uint16_t>(reverse_bits(next[lens[i]]++, lens[i])) : 0;
}
// Sum over 2^-len scaled by 2^15: a complete code gives exactly 32768.
PNGZ_HD uint32_t kraft_sum(const uint8_t *lens, uint32_t n)
{
    uint32_t s = 0;
    for (uint32_t i = 0; i < n; ++i) if (lens[i]) s += 1u << (15 - lens[i]);
    return s;
}

// The lengths of the fixed code (RFC 1951 §3.2.6) in table form: its codes are canonical_codes of these.
PNGZ_HD void fixed_lengths(uint8_t *lit /* kLitTable */, uint8_t *dist /* kDistTable */)
{
    for (uint32_t i = 0; i < kLitTable; ++i) lit[i] = static_cast<uint8_t>(fixed_literal_length(i));
    for (uint32_t i = 0; i < kDistTable; ++i) dist[i] = 5;
}

// ---- tokens -> bits ----------------------------------------------------------------------------------------------------
struct CodeTables {
    const uint16_t *lit_code; const uint8_t *lit_len;
    const uint16_t *dist_code; const uint8_t *dist_len;
};
// The bits of one token, LSB first, at most 48 of them.
PNGZ_HD uint32_t token_code(uint32_t t, const CodeTables &c, uint64_t *bits)
{
    const uint32_t len = token_len(t);
    if (!len) { *bits = c.lit_code[t & 255]; return c.lit_len[t & 255]; }
    uint32_t s, eb, ev, n;
    length_symbol(len, &s, &eb, &ev);
    uint64_t v = c.lit_code[s];
    n = c.lit_len[s];
    v |= static_cast<uint64_t>(ev) << n;
    n += eb;
    distance_symbol(t & 0xFFFF, &s, &eb, &ev);
    v |= static_cast<uint64_t>(c.dist_code[s]) << n;
    n += c.dist_len[s];
    v |= static_cast<uint64_t>(ev) << n;
    n += eb;
    *bits = v;
    return n;
}
PNGZ_HD uint32_t token_bits(uint32_t t, const uint8_t *lit_len, const uint8_t *dist_len)
{
    const uint32_t len = token_len(t);
    if (!len) return lit_len[t & 255];
    uint32_t s, eb, ev, n;
    length_symbol(len, &s, &eb, &ev);
    n = lit_len[s] + eb;
    distance_symbol(t & 0xFFFF, &s, &eb, &ev);
    return n + dist_len[s] + eb;
}
// Bits of the symbols of a block coded with these lengths (the end-of-block symbol is in lit_freq).
PNGZ_HD uint32_t body_bits(const uint32_t *lit_freq, const uint32_t *dist_freq, const uint8_t *lit_len, const uint8_t *dist_len)
{
    uint32_t bits = 0;
    for (uint32_t s = 0; s < kLitSyms; ++s) bits += lit_freq[s] * (lit_len[s] + (s > 256 ? length_symbol_extra(s) : 0u));
    for (uint32_t s = 0; s < kDistSyms; ++s) bits += dist_freq[s] * (dist_len[s] + distance_symbol_extra(s));
    return bits;
}

// ---- the header of a dynamic block (RFC 1951 §3.2.7) ----------------------------------------------------------------
// BFINAL, BTYPE = 10, HLIT, HDIST, HCLEN, the code-length code (at most 7 bits), then the lit_len[0..hlit) and
// dist_len[0..hdist) lengths in its symbols: 0-15 literal, 16 repeats the previous length 3-6 times, 17 / 18 run of
// zeros 3-10 / 11-138 long.  Runs may cross from the literal lengths into the distance lengths, as the format allows.
PNGZ_HD void dynamic_header(BitWriter &bw, uint32_t bfinal, const uint8_t *lit_len, const uint8_t *dist_len, HuffWork &w)
{
    uint32_t hlit = kLitSyms, hdist = kDistSyms;
    while (hlit > 257 && !lit_len[hlit - 1]) --hlit;
    while (hdist > 1 && !dist_len[hdist - 1]) --hdist;
    const uint32_t total = hlit + hdist;
    auto at = [&](uint32_t i) -> uint32_t { return i < hlit ? lit_len[i] : dist_len[i - hlit]; };
    uint32_t nruns = 0, cl_freq[kClSyms];
    for (uint32_t i = 0; i < kClSyms; ++i) cl_freq[i] = 0;
    auto push = [&](uint32_t sym, uint32_t extra) { w.runs[nruns++] = static_cast<uint16_t>(sym | (extra << 8)); ++cl_freq[sym]; };
    for (uint32_t i = 0; i < total;) {
        const uint32_t v = at(i);
        uint32_t run = 1;
        while (i + run < total && at(i + run) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) { const uint32_t r = run < 138 ? run : 138; push(18, r - 11); run -= r; }
            if (run >= 3) { push(17, run - 3); run = 0; }
            while (run--) push(0, 0);
        } else {
            push(v, 0);
            --run;
            while (run >= 3) { const uint32_t r = run < 6 ? run : 6; push(16, r - 3); run -= r; }
            while (run--) push(v, 0);
        }
    }
    uint8_t cl_len[kClSyms];
    uint16_t cl_code[kClSyms];
    huffman_lengths(cl_freq, kClSyms, 7, cl_len, w); // (uses key / sym / bucket / per_length, not runs)
    canonical_codes(cl_len, kClSyms, cl_code);
    const uint8_t order[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t hclen = kClSyms;
    while (hclen > 4 && !cl_len[order[hclen - 1]]) --hclen;
    bw.put(bfinal & 1, 1);
    bw.put(2, 2);
    bw.put(hlit - 257, 5);
    bw.put(hdist - 1, 5);
    bw.put(hclen - 4, 4);
    for (uint32_t i = 0; i < hclen; ++i) bw.put(cl_len[order[i]], 3);
    for (uint32_t i = 0; i < nruns; ++i) {
        const uint32_t s = w.runs[i] & 255, extra = w.runs[i] >> 8;
        bw.put(cl_code[s], cl_len[s]);
        if (s == 16) bw.put(extra, 2);
        else if (s == 17) bw.put(extra, 3);
        else if (s == 18) bw.put(extra, 7);
    }
}

// ---- zlib wrapper ------------------------------------------------------------------------------------------------------
// CMF / FLG for a compression level clamped to 1..9 (FLEVEL 1 for levels up to 2, 2 up to 6, 3 above).
PNGZ_HD void zlib_header(uint32_t level, uint8_t out[2])
{
    level = level < 1 ? 1 : level > 9 ? 9 : level;
    const uint32_t flevel = level <= 2 ? 1 : level <= 6 ? 2 : 3;
    uint32_t flg = flevel << 6;
    flg |= (31 - ((0x78u << 8 | flg) % 31)) % 31;
    out[0] = 0x78;
    out[1] = static_cast<uint8_t>(flg);
}
// Bytes that always hold the zlib stream of len bytes: stored blocks of 65,535, header and checksum.
PNGZ_HD uint64_t stored_bound(uint64_t len) { return len + 5 * ((len + 65534) / 65535) + 6; }

// ---- batches: several streams (segments) in one launch ("segments") -----------------------------------
// A segment is one image's prepared stream.  Its chunks, its window, its blocks' offsets, its zlib header and checksum,
// its IDAT bodies and its CRC pieces are its own: nothing below ever yields an index outside the segment it names.
constexpr uint32_t kSegChunk = 65535;       // input bytes per DEFLATE block (png_deflate.hpp kZChunk)
constexpr uint32_t kSegIdat = 256 * 1024;   // bytes of an IDAT body (kIdatBytes)
constexpr uint32_t kSegPiece = 4096;        // bytes of the stream one CRC value covers (kCrcPiece)
constexpr uint32_t kSegAlign = 16;          // every segment's destination starts on a multiple of this
struct ZSegment {
    uint64_t src;         // its first byte, counted from the launch's data pointer
    uint64_t len;         // its bytes, > 0
    uint64_t dst;         // its framed zlib stream, counted from the launch's destination: a multiple of kSegAlign
    uint32_t first_chunk; // chunks of the segments in front of it
    uint32_t first_piece; // CRC pieces of the segments in front of it, each segment counted by its stored bound
    uint32_t hint_bpp, hint_row;
    uint32_t adler;       // of the segment's bytes (read by the compaction only)
    uint32_t reserved;
};
PNGZ_HD uint64_t seg_chunks(uint64_t len) { return (len + kSegChunk - 1) / kSegChunk; }
PNGZ_HD uint64_t seg_framed_size(uint64_t stream_len) { return stream_len + 12 * ((stream_len + kSegIdat - 1) / kSegIdat); }
PNGZ_HD uint64_t seg_pieces(uint64_t len) { return (stored_bound(len) + kSegPiece - 1) / kSegPiece; } // of the longest stream it can become
PNGZ_HD uint64_t seg_dst_bytes(uint64_t len) { return (seg_framed_size(stored_bound(len)) + kSegAlign - 1) / kSegAlign * kSegAlign; }
// Fills in first_chunk, first_piece and dst of segs[0..n) from their len, and the totals into segs[n] (a table has n + 1
// entries; the last one's src and len are 0).  false: the chunks or pieces do not fit 31 bits.
PNGZ_HD bool seg_layout(ZSegment *segs, uint32_t n)
{
    uint64_t chunk = 0, piece = 0, dst = 0;
    for (uint32_t s = 0; s <= n; ++s) {
        if (chunk > 0x7FFFFFFFull || piece > 0x7FFFFFFFull) return false;
        segs[s].first_chunk = static_cast<uint32_t>(chunk);
        segs[s].first_piece = static_cast<uint32_t>(piece);
        segs[s].dst = dst;
        if (s == n) { segs[s].src = 0; segs[s].len = 0; break; }
        chunk += seg_chunks(segs[s].len);
        piece += seg_pieces(segs[s].len);
        dst += seg_dst_bytes(segs[s].len);
    }
    return true;
}
// The segment that holds global chunk / piece g (g below the table's total): the last one that starts at or before it.
// A search of the n + 1 firsts, not a map with an entry per chunk: the table is what the host uploads anyway, a
// workgroup pays at most 17 uniform loads for it in front of 65,535 bytes of work, and a map would cost the host a loop
// and an upload that grow with the chunks instead of the images.
PNGZ_HD uint32_t seg_of_chunk(const ZSegment *segs, uint32_t n, uint32_t g)
{
    uint32_t lo = 0, hi = n; // segs[lo].first_chunk <= g < segs[hi].first_chunk
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (segs[mid].first_chunk <= g) lo = mid; else hi = mid; }
    return lo;
}
PNGZ_HD uint32_t seg_of_piece(const ZSegment *segs, uint32_t n, uint32_t g)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (segs[mid].first_piece <= g) lo = mid; else hi = mid; }
    return lo;
}
// Chunk `chunk` of a stream of len bytes, all counted from the stream's first byte: where it starts, its bytes, where its
// 32 KiB window starts (never in front of the stream), whether it is the stream's last.
struct ChunkSpan { uint64_t c0, wstart; uint32_t n; bool last; };
PNGZ_HD ChunkSpan chunk_span(uint64_t len, uint64_t chunk)
{
    ChunkSpan r;
    r.c0 = chunk * kSegChunk;
    r.n = static_cast<uint32_t>(len - r.c0 < kSegChunk ? len - r.c0 : kSegChunk);
    r.last = r.c0 + r.n == len;
    r.wstart = r.c0 > kWindow ? r.c0 - kWindow : 0;
    return r;
}
// Piece `piece` of a segment whose zlib stream has stream_len bytes: its first byte in the stream and its bytes (0: the
// piece lies behind the stream's end and has no value).
PNGZ_HD uint32_t piece_span(uint64_t stream_len, uint64_t piece, uint64_t *s0)
{
    *s0 = piece * kSegPiece;
    if (*s0 >= stream_len) return 0;
    return static_cast<uint32_t>(stream_len - *s0 < kSegPiece ? stream_len - *s0 : kSegPiece);
}
// Where byte s of a zlib stream lies in its destination as IDAT bodies: 8 bytes in front of every body, 4 behind.
PNGZ_HD uint64_t seg_framed_offset(uint64_t s) { return s + 8 + 12 * (s / kSegIdat); }

// ---- CRC-32 (reflected 0xEDB88320) -----------------------------------------------------------------------------------
PNGZ_HD uint32_t crc32_table_entry(uint32_t i)
{
    for (int k = 0; k < 8; ++k) i = (i & 1) ? (i >> 1) ^ 0xEDB88320u : i >> 1;
    return i;
}
PNGZ_HD uint32_t crc32_bytes(uint32_t crc, const uint8_t *p, uint64_t n) // zlib.crc32(p, crc)
{
    crc = ~crc;
    for (uint64_t i = 0; i < n; ++i) crc = crc32_table_entry((crc ^ p[i]) & 255) ^ (crc >> 8);
    return ~crc;
}
// a * b mod P over GF(2), polynomials in the CRC's reflected bit order (x^0 is bit 31)
PNGZ_HD uint32_t crc32_multiply(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
PNGZ_HD uint32_t crc32_x_pow(uint64_t n) // x^n mod P
{
    uint32_t r = 1u << 31, b = 1u << 30;
    for (; n; n >>= 1) { if (n & 1) r = crc32_multiply(r, b); b = crc32_multiply(b, b); }
    return r;
}
// crc32(A || B) from crc32(A), crc32(B) and B's length: shift A's value by 8 * len_b bits and combine.
PNGZ_HD uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc32_multiply(crc32_x_pow(8 * len_b), crc_a) ^ crc_b; }

} // namespace pixo_pngz
