// TEST HARNESS — the host build of pixo_amd/csrc/png_deflate_math.h: the length limiter, the header coder, the bit
// writer and the CRC combine on their own, and one DEFLATE block assembled from a token list in the steps the kernel
// (png_deflate.hip) takes after its parse.
#include <cstring>
#include <vector>

#include "../../pixo_amd/csrc/png_deflate_math.h"

using namespace pixo_pngz;

extern "C" {

void emu_huffman_lengths(const uint32_t *freq, uint32_t n, uint32_t max_bits, uint8_t *lens)
{
    HuffWork w;
    huffman_lengths(freq, n, max_bits, lens, w);
}
uint32_t emu_kraft(const uint8_t *lens, uint32_t n) { return kraft_sum(lens, n); }
void emu_canonical_codes(const uint8_t *lens, uint32_t n, uint16_t *codes) { canonical_codes(lens, n, codes); }
void emu_symbols(uint32_t len, uint32_t dist, uint32_t *out6)
{
    length_symbol(len, out6, out6 + 1, out6 + 2);
    distance_symbol(dist, out6 + 3, out6 + 4, out6 + 5);
}
uint32_t emu_crc32(uint32_t crc, const uint8_t *p, uint64_t n) { return crc32_bytes(crc, p, n); }
uint32_t emu_crc32_combine(uint32_t a, uint32_t b, uint64_t len_b) { return crc32_combine(a, b, len_b); }
void emu_zlib_header(uint32_t level, uint8_t *out2) { zlib_header(level, out2); }
uint64_t emu_stored_bound(uint64_t n) { return stored_bound(n); }

// One block for `tokens` (token_match / literal bytes) whose bytes are data[0..n): mode 0 stored, 1 fixed, 2 dynamic,
// 3 the smallest as the kernel chooses.  Not final: followed by the empty stored block.  Returns the bytes written; *chosen
// receives the form.
uint32_t emu_block(const uint32_t *tokens, uint32_t ntok, const uint8_t *data, uint32_t n, uint32_t mode, uint32_t last, uint8_t *out,
                   uint32_t *chosen)
{
    uint32_t lit_freq[kLitTable] = {0}, dist_freq[kDistTable] = {0};
    lit_freq[256] = 1;
    for (uint32_t i = 0; i < ntok; ++i) {
        const uint32_t l = token_len(tokens[i]);
        uint32_t s, eb, ev;
        if (l) {
            length_symbol(l, &s, &eb, &ev); ++lit_freq[s];
            distance_symbol(tokens[i] & 0xFFFF, &s, &eb, &ev); ++dist_freq[s];
        } else ++lit_freq[tokens[i] & 255];
    }
    uint8_t lit_len[kLitTable] = {0}, dist_len[kDistTable] = {0}, fix_lit[kLitTable], fix_dist[kDistTable];
    uint16_t lit_code[kLitTable], dist_code[kDistTable];
    HuffWork w;
    huffman_lengths(lit_freq, kLitSyms, 15, lit_len, w);
    huffman_lengths(dist_freq, kDistSyms, 15, dist_len, w);
    fixed_lengths(fix_lit, fix_dist);
    std::vector<uint8_t> header(kHeaderBytes, 0);
    BitWriter hw(header.data());
    dynamic_header(hw, last, lit_len, dist_len, w);
    const uint32_t head = hw.bit_count();
    hw.flush();
    const uint32_t dyn = head + body_bits(lit_freq, dist_freq, lit_len, dist_len), fix = 3 + body_bits(lit_freq, dist_freq, fix_lit, fix_dist);
    const uint32_t dyn_bytes = last ? (dyn + 7) / 8 : (dyn + 3 + 7) / 8 + 4, fix_bytes = last ? (fix + 7) / 8 : (fix + 3 + 7) / 8 + 4;
    if (mode == 3) {
        uint32_t bytes = n + 5;
        mode = 0;
        if (fix_bytes < bytes) { mode = 1; bytes = fix_bytes; }
        if (dyn_bytes < bytes) { mode = 2; bytes = dyn_bytes; }
    }
    *chosen = mode;
    if (mode == 0) {
        out[0] = last ? 1 : 0;
        out[1] = n & 255; out[2] = n >> 8; out[3] = ~n & 255; out[4] = (~n >> 8) & 255;
        std::memcpy(out + 5, data, n);
        return n + 5;
    }
    const uint32_t bytes = mode == 1 ? fix_bytes : dyn_bytes;
    std::memset(out, 0, bytes);
    BitWriter bw(out);
    if (mode == 1) {
        std::memcpy(lit_len, fix_lit, sizeof(fix_lit));
        std::memcpy(dist_len, fix_dist, sizeof(fix_dist));
        bw.put((last ? 1u : 0u) | 2u, 3);
    } else {
        for (uint32_t i = 0; i < head / 8; ++i) bw.put(header[i], 8);
        if (head % 8) bw.put(header[head / 8], head % 8);
    }
    canonical_codes(lit_len, kLitTable, lit_code);
    canonical_codes(dist_len, kDistTable, dist_code);
    const CodeTables codes{lit_code, lit_len, dist_code, dist_len};
    for (uint32_t i = 0; i < ntok; ++i) {
        uint64_t v;
        const uint32_t k = token_code(tokens[i], codes, &v);
        if (k != token_bits(tokens[i], lit_len, dist_len)) return 0;
        bw.put(static_cast<uint32_t>(v), k < 32 ? k : 32);
        if (k > 32) bw.put(static_cast<uint32_t>(v >> 32), k - 32);
    }
    bw.put(lit_code[256], lit_len[256]);
    if (bw.bit_count() != (mode == 1 ? fix : dyn)) return 0;
    if (!last) { bw.put(0, 3); bw.flush(); bw.put(0, 16); bw.put(0xFFFF, 16); }
    bw.flush();
    return bw.pos == bytes ? bytes : 0;
}

} // extern "C"
