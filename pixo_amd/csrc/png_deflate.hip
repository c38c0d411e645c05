// png_deflate.hip — DEFLATE on the device for the PNG whole-file path.
//
// The stream is cut into chunks of at most 65,535 bytes; one workgroup of 1024 lanes turns one chunk into one DEFLATE block
// in the chunk's slot.  Every block but the last is followed by an empty stored block (000, pad, 00 00 FF FF), so every
// block starts on a byte boundary and joining them is a byte compaction.  Per chunk:
//   1. match finding, one position per lane and sub-step of 1024 positions: a 4-byte hash table in LDS (latest position,
//      filled with atomicMax after all lanes of the sub-step have looked up, so the result does not depend on scheduling),
//      seeded with the 32 KiB in front of the chunk, plus the distances 1, hint_bpp, hint_row tried explicitly;
//   2. greedy parse over next[p] = p + max(len[p], 1): every lane resolves where each position of its 64-position segment
//      leaves the segment (in LDS, back to front), ONE lane then hops from segment to segment (at most 1024 hops), and
//      every lane walks its own segment from the entry it was given — tokens compacted in place, histograms by LDS atomics;
//   3. code lengths (literal/length and distance trees on one lane each), dynamic header, sizes of the three forms;
//   4. token bit lengths, exclusive scan, LSB-first packing into LDS with atomicOr, vector stores to the slot.
// The high effort (template argument) replaces step 1 and changes the next[] of step 2; steps 2 to 4 are the same code:
//   1a. links: the window and the chunk are walked in sub-steps of kZEffortSubstep positions by ONE wavefront (the hashes
//       of 16,384 positions at a time are put into LDS by all lanes first): every position reads the head of its hash,
//       then every position of the sub-step inserts itself; the distance to the head seen is the position's link, a
//       u16 in global memory.  Links depend on hashes only, never on match lengths;
//   1b. every position in parallel, as in step 1: distance 1, hint_bpp, up to kZEffortProbes entries along the links, hint_row;
//   1c. one-step lazy: a position whose successor has a strictly longer match becomes a literal, so next[p] = p + 1 there
//       and step 2 runs on the tokens as they then are.
// Only vector stores write device memory.
#include <hip/hip_runtime.h>

#include "png_deflate.hpp"

namespace pixo_dev {
using namespace pixo_pngz;

namespace {
constexpr uint32_t kThreads = 1024, kSeg = 64, kHashBits = 14, kNoEntry = 0xFFFF;
constexpr uint32_t kLinkPiece = 16384, kNoHash = 0xFFFF; // high effort: positions whose hashes LDS holds at a time
static_assert(kLinkPiece % kZEffortSubstep == 0 && kLinkPiece % kThreads == 0 && kWindow % kLinkPiece == 0, "whole sub-steps per piece");
static_assert(kThreads * kSeg >= kZChunk, "a lane per segment");

__device__ __forceinline__ uint32_t load_u32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint64_t load_u64(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
__device__ __forceinline__ uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }

// bytes that agree at p and q (q < p), at most max_len; reads p[0..max_len) only
__device__ __forceinline__ uint32_t match_length(const uint8_t *p, const uint8_t *q, uint32_t max_len)
{
    uint32_t k = 0;
    while (k + 8 <= max_len) {
        const uint64_t x = load_u64(p + k) ^ load_u64(q + k);
        if (x) return k + (static_cast<uint32_t>(__builtin_ctzll(x)) >> 3);
        k += 8;
    }
    while (k < max_len && p[k] == q[k]) ++k;
    return k;
}

struct ChunkShared {
    union {
        uint32_t hash[1u << kHashBits]; // position - window start + 1 of the latest occurrence, 0: none
        uint16_t exit[65536];           // parse: where the path from p leaves p's segment
        uint32_t out[32768];            // the block being packed
        struct {
            uint32_t head[1u << kHashBits]; // the same table as `hash`
            uint16_t hash_of[kLinkPiece];   // high effort, links: the hash of every position of the piece, kNoHash: none
        } link;
    } big;
    uint16_t entry[kThreads];
    uint32_t scan[kThreads];
    uint32_t lit_freq[kLitTable], dist_freq[kDistTable];
    uint16_t lit_code[kLitTable], dist_code[kDistTable];
    uint8_t lit_len[kLitTable], dist_len[kDistTable];
    uint8_t fix_lit_len[kLitTable], fix_dist_len[kDistTable];
    HuffWork work[2];
    uint8_t header[kHeaderBytes];
    unsigned long long sum_a, sum_b;
    uint32_t mode, header_bits, block_bytes;
};

// One chunk of one stream: `data` is the stream's first byte, `len` its bytes, `chunk` the chunk's number in the stream; tok,
// slot, info and prev are the chunk's own places in the scratch.  The stream is one segment of the launch's table
// (deflate_chunk_kernel): the window, `last`, the hash seeding and the links never leave it.
template <bool kHigh>
__device__ __forceinline__ void deflate_chunk(const uint8_t *__restrict__ data, uint64_t len, uint32_t hint_bpp, uint32_t hint_row, uint64_t chunk,
                                              uint32_t *__restrict__ tok, uint8_t *__restrict__ slot, ZChunkInfo *__restrict__ info,
                                              uint16_t *__restrict__ prev)
{
    __shared__ ChunkShared s;
    const uint32_t tid = threadIdx.x;
    const ChunkSpan span = chunk_span(len, chunk);
    const uint64_t c0 = span.c0, wstart = span.wstart;
    const uint32_t n = span.n; // 1..65535
    const bool last = span.last;

    for (uint32_t i = tid; i < (1u << kHashBits); i += kThreads) s.big.hash[i] = 0;
    if (tid < kLitTable) s.lit_freq[tid] = tid == 256 ? 1u : 0u; // the end-of-block symbol
    if (tid < kDistTable) s.dist_freq[tid] = 0;
    if (tid == 0) { s.sum_a = 0; s.sum_b = 0; }
    __syncthreads();

    { // Adler-32 partial sums of the chunk
        unsigned long long a = 0, b = 0;
        for (uint32_t p = tid; p < n; p += kThreads) { const uint32_t v = data[c0 + p]; a += v; b += static_cast<unsigned long long>(n - p) * v; }
        for (int off = 32; off; off >>= 1) { a += __shfl_down(a, off); b += __shfl_down(b, off); }
        if ((tid & 63) == 0) { atomicAdd(&s.sum_a, a); atomicAdd(&s.sum_b, b); }
    }
    if constexpr (kHigh) {
        const uint32_t wlen = static_cast<uint32_t>(c0 - wstart), total = wlen + n; // 0 or kWindow; <= kZPrevStride
        __syncthreads();
        // ---- 1a. links ----
        for (uint32_t piece = 0; piece < total; piece += kLinkPiece) {
            for (uint32_t i = tid; i < kLinkPiece; i += kThreads) {
                const uint32_t r = piece + i;
                uint32_t hv = kNoHash;
                if (r < total) { // as in step 1: the window's positions hash while four bytes of the stream are left, the chunk's while four of the chunk are
                    const uint64_t a = wstart + r;
                    if (r < wlen ? a + 4 <= len : r - wlen + 4 <= n) hv = hash4(load_u32(data + a));
                }
                s.big.link.hash_of[i] = static_cast<uint16_t>(hv);
            }
            __syncthreads();
            if (tid < 64) { // one wavefront: its LDS operations take effect in program order, so no barrier is needed between sub-steps
                const uint32_t end = total - piece < kLinkPiece ? total - piece : kLinkPiece;
                for (uint32_t sub = 0; sub < end; sub += kZEffortSubstep) {
                    uint32_t hv[kZEffortSubstep / 64], seen[kZEffortSubstep / 64];
#pragma unroll
                    for (uint32_t j = 0; j < kZEffortSubstep / 64; ++j) {
                        hv[j] = s.big.link.hash_of[sub + 64 * j + tid];
                        seen[j] = hv[j] != kNoHash ? __hip_atomic_load(&s.big.link.head[hv[j]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0;
                    }
                    __builtin_amdgcn_wave_barrier(); // every look-up of the sub-step is issued before its first insert
#pragma unroll
                    for (uint32_t j = 0; j < kZEffortSubstep / 64; ++j) {
                        const uint32_t r = piece + sub + 64 * j + tid;
                        if (hv[j] != kNoHash) atomicMax(&s.big.link.head[hv[j]], r + 1);
                        if (r < total) prev[r] = static_cast<uint16_t>(chain_link(r, seen[j])); // (kWindow itself fits 16 bits)
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
            __syncthreads();
        }
        // ---- 1b, 1c. the best match at every position; a position gives way to a longer match at the next ----
        for (uint32_t base = 0; base < n; base += kThreads) {
            const uint32_t p = base + tid;
            const bool active = p < n;
            const uint64_t a = c0 + p;
            uint32_t best_len = 0, best_dist = 0;
            if (active) {
                const uint32_t max_len = n - p < kMaxMatch ? n - p : kMaxMatch;
                auto attempt = [&](uint64_t d) {
                    if (d == 0 || d > kWindow || d > a || best_len == max_len) return;
                    const uint32_t l = match_length(data + a, data + a - d, max_len);
                    if (l > best_len || (l == best_len && d < best_dist)) { best_len = l; best_dist = static_cast<uint32_t>(d); }
                };
                if (max_len >= kMinMatch) {
                    attempt(1);
                    if (hint_bpp > 1) attempt(hint_bpp);
                    uint32_t dist = 0;
                    for (uint32_t k = 0; k < kZEffortProbes && best_len < max_len; ++k) {
                        dist = chain_step(dist, prev[wlen + p - dist]);
                        if (!dist) break;
                        attempt(dist);
                    }
                    if (hint_row > 1 && hint_row != hint_bpp) attempt(hint_row);
                }
                best_len = kept_length(best_len, best_dist);
            }
            s.scan[tid] = best_len; // (0 beyond the chunk's end)
            __syncthreads();
            if (active) {
                const uint32_t len_next = tid + 1 < kThreads ? s.scan[tid + 1] : 0; // the last lane's successor: settled by lane 0 of the next round
                tok[p] = best_len && !lazy_defers(best_len, len_next) ? token_match(best_len, best_dist) : data[a];
            }
            __syncthreads(); // tok[base - 1] is written; s.scan is free again
            if (tid == 0 && base && lazy_defers(token_len(tok[base - 1]), best_len)) tok[base - 1] = data[a - 1];
        }
        __syncthreads();
    } else { // effort 0: step 1 as it has always been
        // the window in front of the chunk
        for (uint64_t a = wstart + tid; a < c0; a += kThreads)
            if (a + 4 <= len) atomicMax(&s.big.hash[hash4(load_u32(data + a))], static_cast<uint32_t>(a - wstart) + 1);
        __syncthreads();

        // ---- 1. the best match at every position ----
        for (uint32_t base = 0; base < n; base += kThreads) {
            const uint32_t p = base + tid;
            const bool active = p < n;
            const uint64_t a = c0 + p;
            uint32_t best_len = 0, best_dist = 0, hv = 0;
            bool hashed = false;
            if (active) {
                const uint32_t max_len = n - p < kMaxMatch ? n - p : kMaxMatch;
                uint32_t cand = 0;
                if (p + 4 <= n) { hashed = true; hv = hash4(load_u32(data + a)); cand = s.big.hash[hv]; }
                auto attempt = [&](uint64_t d) {
                    if (d == 0 || d > kWindow || d > a || best_len == max_len) return;
                    const uint32_t l = match_length(data + a, data + a - d, max_len);
                    if (l > best_len || (l == best_len && d < best_dist)) { best_len = l; best_dist = static_cast<uint32_t>(d); }
                };
                if (max_len >= kMinMatch) {
                    attempt(1);
                    if (hint_bpp > 1) attempt(hint_bpp);
                    if (cand) attempt(a - (wstart + cand - 1));
                    if (hint_row > 1 && hint_row != hint_bpp) attempt(hint_row);
                }
                if (best_len < kMinMatch || (best_len == kMinMatch && best_dist > 4096)) best_len = 0; // dearer than its literals
            }
            __syncthreads(); // every lane of the sub-step has looked up
            if (hashed) atomicMax(&s.big.hash[hv], static_cast<uint32_t>(a - wstart) + 1);
            if (active) tok[p] = best_len ? token_match(best_len, best_dist) : data[a];
            __syncthreads();
        }
    } // effort 0

    // ---- 2. parse: greedy over the tokens as they stand (the high effort has made its deferred positions literals) ----
    for (uint32_t p = tid; p < n; p += kThreads) {
        const uint32_t l = token_len(tok[p]);
        const uint32_t e = p + (l ? l : 1);
        s.big.exit[p] = static_cast<uint16_t>(e < n ? e : n);
    }
    s.entry[tid] = kNoEntry;
    __syncthreads();
    const uint32_t lo = tid * kSeg, hi = lo + kSeg < n ? lo + kSeg : n;
    for (uint32_t p = hi; p > lo; --p) { // (hi <= lo: nothing of the chunk in this segment)
        const uint32_t e = s.big.exit[p - 1];
        if (e < hi) s.big.exit[p - 1] = s.big.exit[e];
    }
    __syncthreads();
    if (tid == 0)
        for (uint32_t pos = 0; pos < n; pos = s.big.exit[pos]) s.entry[pos / kSeg] = static_cast<uint16_t>(pos);
    __syncthreads();
    uint32_t count = 0; // tokens of this lane's segment, compacted to tok[lo .. lo + count)
    if (s.entry[tid] != kNoEntry) {
        for (uint32_t pos = s.entry[tid]; pos < hi;) {
            const uint32_t t = tok[pos];
            const uint32_t l = token_len(t);
            if (l) {
                uint32_t sym, eb, ev;
                length_symbol(l, &sym, &eb, &ev);
                atomicAdd(&s.lit_freq[sym], 1u);
                distance_symbol(t & 0xFFFF, &sym, &eb, &ev);
                atomicAdd(&s.dist_freq[sym], 1u);
            } else {
                atomicAdd(&s.lit_freq[t & 255], 1u);
            }
            tok[lo + count++] = t; // lo + count <= pos: behind the read
            pos += l ? l : 1;
        }
    }
    __syncthreads();

    // ---- 3. codes and the form of the block ----
    if (tid == 0) huffman_lengths(s.lit_freq, kLitSyms, 15, s.lit_len, s.work[0]);
    if (tid == 64) huffman_lengths(s.dist_freq, kDistSyms, 15, s.dist_len, s.work[1]);
    if (tid == 128) fixed_lengths(s.fix_lit_len, s.fix_dist_len);
    __syncthreads();
    if (tid == 0) {
        s.lit_len[286] = s.lit_len[287] = 0;
        s.dist_len[30] = s.dist_len[31] = 0;
        BitWriter bw(s.header);
        dynamic_header(bw, last, s.lit_len, s.dist_len, s.work[0]);
        const uint32_t head = bw.bit_count();
        bw.flush();
        const uint32_t dyn = head + body_bits(s.lit_freq, s.dist_freq, s.lit_len, s.dist_len);
        const uint32_t fix = 3 + body_bits(s.lit_freq, s.dist_freq, s.fix_lit_len, s.fix_dist_len);
        // bytes in the slot: a block that is not the last is followed by the empty stored block
        const uint32_t dyn_bytes = last ? (dyn + 7) / 8 : (dyn + 3 + 7) / 8 + 4;
        const uint32_t fix_bytes = last ? (fix + 7) / 8 : (fix + 3 + 7) / 8 + 4;
        const uint32_t stored_bytes = n + 5;
        uint32_t mode = 0, bytes = stored_bytes;
        if (fix_bytes < bytes) { mode = 1; bytes = fix_bytes; }
        if (dyn_bytes < bytes) { mode = 2; bytes = dyn_bytes; }
        s.mode = mode;
        s.block_bytes = bytes;
        s.header_bits = mode == 2 ? head : 3;
        if (mode == 1) { s.header[0] = static_cast<uint8_t>((last ? 1u : 0u) | 2u); } // BFINAL, BTYPE = 01
        *info = ZChunkInfo{bytes, mode, s.sum_a, s.sum_b};
    }
    __syncthreads();
    const uint32_t mode = s.mode, block_bytes = s.block_bytes;
    const uint32_t words = (block_bytes + 3) / 4; // <= kZSlot / 4
    uint32_t *slot_words = reinterpret_cast<uint32_t *>(slot);
    if (mode == 0) { // stored: BFINAL + 00, LEN, NLEN, the bytes
        for (uint32_t w = tid; w < words; w += kThreads) {
            uint32_t v = 0;
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t i = 4 * w + k;
                uint32_t byte = 0;
                if (i == 0) byte = last ? 1u : 0u;
                else if (i == 1) byte = n & 255;
                else if (i == 2) byte = n >> 8;
                else if (i == 3) byte = ~n & 255;
                else if (i == 4) byte = (~n >> 8) & 255;
                else if (i < n + 5) byte = data[c0 + i - 5];
                v |= byte << (8 * k);
            }
            slot_words[w] = v;
        }
        return;
    }
    if (mode == 1 && tid < kLitTable) s.lit_len[tid] = s.fix_lit_len[tid];
    if (mode == 1 && tid < kDistTable) s.dist_len[tid] = s.fix_dist_len[tid];
    __syncthreads();
    if (tid == 0) canonical_codes(s.lit_len, kLitTable, s.lit_code);
    if (tid == 64) canonical_codes(s.dist_len, kDistTable, s.dist_code);

    // ---- 4. pack ----
    uint32_t bits = 0;
    for (uint32_t j = 0; j < count; ++j) bits += token_bits(tok[lo + j], s.lit_len, s.dist_len);
    s.scan[tid] = bits;
    for (uint32_t w = tid; w < words + 1; w += kThreads) s.big.out[w] = 0; // words + 1 <= 32768
    __syncthreads();
    for (uint32_t step = 1; step < kThreads; step <<= 1) { // inclusive scan
        const uint32_t add = tid >= step ? s.scan[tid - step] : 0;
        __syncthreads();
        s.scan[tid] += add;
        __syncthreads();
    }
    const uint32_t header_bits = s.header_bits;
    const uint32_t body_end = header_bits + s.scan[kThreads - 1]; // where the end-of-block symbol goes
    for (uint32_t i = tid; i < (header_bits + 7) / 8; i += kThreads) atomicOr(&s.big.out[i >> 2], static_cast<uint32_t>(s.header[i]) << (8 * (i & 3)));
    auto put = [&](uint32_t at, uint64_t v) { // v: at most 48 bits
        const uint32_t w = at >> 5, sh = at & 31;
        const uint32_t w0 = static_cast<uint32_t>(v << sh);
        const uint64_t rest = sh ? v >> (32 - sh) : v >> 32;
        if (w0) atomicOr(&s.big.out[w], w0);
        if (static_cast<uint32_t>(rest)) atomicOr(&s.big.out[w + 1], static_cast<uint32_t>(rest));
        if (rest >> 32) atomicOr(&s.big.out[w + 2], static_cast<uint32_t>(rest >> 32));
    };
    const CodeTables codes{s.lit_code, s.lit_len, s.dist_code, s.dist_len};
    uint32_t at = header_bits + s.scan[tid] - bits;
    for (uint32_t j = 0; j < count; ++j) {
        uint64_t v;
        const uint32_t k = token_code(tok[lo + j], codes, &v);
        put(at, v);
        at += k;
    }
    if (tid == 0) {
        put(body_end, s.lit_code[256]);
        if (!last) { // 000 and the padding are zero bits already; LEN = 0, NLEN = FFFF
            const uint32_t i = (body_end + s.lit_len[256] + 3 + 7) / 8 + 2;
            atomicOr(&s.big.out[i >> 2], 0xFFu << (8 * (i & 3)));
            atomicOr(&s.big.out[(i + 1) >> 2], 0xFFu << (8 * ((i + 1) & 3)));
        }
    }
    __syncthreads();
    for (uint32_t w = tid; w < words; w += kThreads) slot_words[w] = s.big.out[w];
}

// Workgroup b finds its segment in the table (png_deflate_math.h seg_of_chunk: uniform loads, none for a table of one) and
// works on chunk b - first_chunk of that segment's stream; the scratch is indexed by b.
template <bool kHigh>
__global__ __launch_bounds__(kThreads) void deflate_chunk_kernel(const uint8_t *__restrict__ data, const ZSegment *__restrict__ segs, uint32_t nseg,
                                                                 uint32_t *__restrict__ tok_all, uint8_t *__restrict__ slots,
                                                                 ZChunkInfo *__restrict__ info, uint16_t *__restrict__ prev_all)
{
    const uint32_t b = blockIdx.x;
    const ZSegment sg = segs[seg_of_chunk(segs, nseg, b)];
    deflate_chunk<kHigh>(data + sg.src, sg.len, sg.hint_bpp, sg.hint_row, b - sg.first_chunk, tok_all + static_cast<uint64_t>(b) * kZTokStride,
                         slots + static_cast<uint64_t>(b) * kZSlot, info + b, kHigh ? prev_all + static_cast<uint64_t>(b) * kZPrevStride : nullptr);
}

__device__ __forceinline__ uint64_t framed_offset(uint64_t s, bool framed) { return framed ? seg_framed_offset(s) : s; }

// One chunk's block from its slot to stream bytes [start, end) of the destination; the stream's first chunk also writes the
// zlib header, its last the checksum.
__device__ __forceinline__ void compact_chunk(const uint8_t *__restrict__ src, uint64_t start, uint64_t end, bool first_chunk, bool last_chunk,
                                              uint32_t header, uint32_t adler, uint8_t *__restrict__ dst, bool framed)
{
    const uint32_t tid = threadIdx.x;
    if (first_chunk && tid < 2) dst[framed_offset(tid, framed)] = static_cast<uint8_t>(header >> (8 * tid));
    if (last_chunk && tid < 4) dst[framed_offset(end + tid, framed)] = static_cast<uint8_t>(adler >> (8 * (3 - tid))); // big endian
    // stream offsets that are multiples of 4 are 4-byte aligned addresses when the destination's first one is: an aligned
    // word never crosses an IDAT boundary (a multiple of 4) and never belongs to two blocks.  (A segment of a batch starts
    // on a multiple of 16 of an aligned buffer, so the test and the argument hold for each segment by itself.)
    const bool aligned = (reinterpret_cast<uintptr_t>(dst + framed_offset(0, framed)) & 3) == 0;
    uint64_t first = (start + 3) & ~uint64_t{3}, lastw = end & ~uint64_t{3};
    if (!aligned || first >= lastw) first = lastw = end; // bytes only
    for (uint64_t sb = start + tid; sb < first; sb += 256) dst[framed_offset(sb, framed)] = src[sb - start];
    for (uint64_t sw = first + 4 * static_cast<uint64_t>(tid); sw < lastw; sw += 4 * 256)
        *reinterpret_cast<uint32_t *>(dst + framed_offset(sw, framed)) = load_u32(src + (sw - start));
    for (uint64_t sb = lastw + tid; sb < end; sb += 256) dst[framed_offset(sb, framed)] = src[sb - start];
}

// Scan: one workgroup per segment, the offsets restart at every segment (offsets[b]: the bytes of the segment's blocks in
// front of global chunk b), totals[s]: the bytes of all blocks of segment s.
__global__ __launch_bounds__(1024) void deflate_scan_kernel(const ZChunkInfo *__restrict__ info, const ZSegment *__restrict__ segs,
                                                                unsigned long long *__restrict__ offsets, unsigned long long *__restrict__ totals)
{
    __shared__ unsigned long long part[1024];
    const uint32_t tid = threadIdx.x, sg = blockIdx.x;
    const uint64_t base = segs[sg].first_chunk, chunks = segs[sg + 1].first_chunk - base;
    const uint64_t per = (chunks + 1023) / 1024;
    const uint64_t c_lo = tid * per < chunks ? tid * per : chunks, c_hi = c_lo + per < chunks ? c_lo + per : chunks;
    unsigned long long sum = 0;
    for (uint64_t c = c_lo; c < c_hi; ++c) sum += info[base + c].bytes;
    part[tid] = sum;
    __syncthreads();
    for (uint32_t step = 1; step < 1024; step <<= 1) {
        const unsigned long long add = tid >= step ? part[tid - step] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    unsigned long long at = part[tid] - sum;
    for (uint64_t c = c_lo; c < c_hi; ++c) { offsets[base + c] = at; at += info[base + c].bytes; }
    if (tid == 1023) totals[sg] = part[1023];
}

// Compaction: workgroup b moves global chunk b's block to its segment's own destination.
__global__ __launch_bounds__(256) void deflate_compact_kernel(const uint8_t *__restrict__ slots, const ZChunkInfo *__restrict__ info,
                                                              const unsigned long long *__restrict__ offsets, const ZSegment *__restrict__ segs,
                                                              uint32_t nseg, uint32_t header, uint8_t *__restrict__ dst, bool framed)
{
    const uint32_t b = blockIdx.x, sg = seg_of_chunk(segs, nseg, b);
    const uint64_t start = 2 + offsets[b];
    compact_chunk(slots + static_cast<uint64_t>(b) * kZSlot, start, start + info[b].bytes, b == segs[sg].first_chunk, b + 1 == segs[sg + 1].first_chunk,
                  header, segs[sg].adler, dst + segs[sg].dst, framed);
}

// Slicing by 4: one aligned word of the stream per step
__device__ __forceinline__ void crc_tables(uint32_t (*table)[256])
{
    for (uint32_t i = threadIdx.x; i < 256; i += 64) {
        uint32_t v = crc32_table_entry(i);
        table[0][i] = v;
        for (int k = 1; k < 4; ++k) { v = crc32_table_entry(v & 255) ^ (v >> 8); table[k][i] = v; }
    }
    __syncthreads();
}
__device__ __forceinline__ uint32_t crc_of_piece(const uint8_t *p, uint32_t nbytes, const uint32_t (*table)[256])
{
    uint32_t crc = 0xFFFFFFFFu, i = 0;
    for (; i + 4 <= nbytes; i += 4) {
        crc ^= *reinterpret_cast<const uint32_t *>(p + i);
        crc = table[3][crc & 255] ^ table[2][(crc >> 8) & 255] ^ table[1][(crc >> 16) & 255] ^ table[0][crc >> 24];
    }
    for (; i < nbytes; ++i) crc = table[0][(crc ^ p[i]) & 255] ^ (crc >> 8);
    return ~crc;
}
// The grid covers every segment's pieces by its stored bound, so that the host need not know the streams' lengths to launch
// it; a lane reads its segment's real length from the scan's totals, and pieces behind the end write nothing.
__global__ __launch_bounds__(64) void deflate_crc_kernel(const uint8_t *__restrict__ dst, const ZSegment *__restrict__ segs, uint32_t nseg,
                                                         const unsigned long long *__restrict__ totals, uint32_t *__restrict__ crcs)
{
    __shared__ uint32_t table[4][256];
    crc_tables(table);
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * 64 + threadIdx.x;
    if (g >= segs[nseg].first_piece) return;
    const uint32_t sg = seg_of_piece(segs, nseg, static_cast<uint32_t>(g));
    uint64_t s0;
    const uint32_t nbytes = piece_span(2 + totals[sg] + 4, g - segs[sg].first_piece, &s0);
    if (!nbytes) return;
    crcs[g] = crc_of_piece(dst + segs[sg].dst + framed_offset(s0, true), nbytes, table);
}
} // namespace

hipError_t launch_deflate(const void *d_data, const ZSegment *d_segs, uint32_t nseg, uint32_t chunks, uint32_t effort, uint32_t *d_tok,
                          uint16_t *d_prev, uint8_t *d_slots, ZChunkInfo *d_info, hipStream_t stream)
{
    if (nseg == 0 || chunks == 0 || chunks > 0x7FFFFFFFu || effort > 1 || (effort && !d_prev)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(effort ? deflate_chunk_kernel<true> : deflate_chunk_kernel<false>, dim3(chunks), dim3(kThreads), 0, stream,
                       static_cast<const uint8_t *>(d_data), d_segs, nseg, d_tok, d_slots, d_info, d_prev);
    return hipGetLastError();
}

hipError_t launch_deflate_finish(const uint8_t *d_slots, const ZChunkInfo *d_info, const ZSegment *d_segs, uint32_t nseg, uint32_t chunks,
                                 uint32_t pieces, uint32_t header, unsigned long long *d_offsets, unsigned long long *d_totals, uint8_t *d_dst,
                                 bool framed, uint32_t *d_crc, hipStream_t stream)
{
    // (framed: word stores and the CRC's word loads at every segment's multiple of kSegAlign; unframed: compact_chunk looks at the pointer)
    if (nseg == 0 || chunks == 0 || pieces == 0 || (framed && reinterpret_cast<uintptr_t>(d_dst) % kSegAlign) || (d_crc && !framed)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(deflate_scan_kernel, dim3(nseg), dim3(1024), 0, stream, d_info, d_segs, d_offsets, d_totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(deflate_compact_kernel, dim3(chunks), dim3(256), 0, stream, d_slots, d_info, d_offsets, d_segs, nseg, header, d_dst, framed);
    if ((e = hipGetLastError()) != hipSuccess || !d_crc) return e;
    hipLaunchKernelGGL(deflate_crc_kernel, dim3((pieces + 63) / 64), dim3(64), 0, stream, d_dst, d_segs, nseg, d_totals, d_crc);
    return hipGetLastError();
}

} // namespace pixo_dev
