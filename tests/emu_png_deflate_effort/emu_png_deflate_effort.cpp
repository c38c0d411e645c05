// TEST HARNESS ONLY — the high effort of the device DEFLATE (pixo_amd/csrc/png_deflate.hip, steps 1a to 1c) walked on the
// host, one position after the other, with the functions the kernel uses for its links, its chains and its lazy rule
// (png_deflate_math.h): what the links hold as 16-bit distances, where a chain stops, which positions give way.
#include <cstring>
#include <vector>

#include "../../pixo_amd/csrc/png_deflate_math.h"

using namespace pixo_pngz;

namespace {
constexpr uint32_t kChunk = 65535, kHashBits = 14;

uint32_t hash4(const uint8_t *p)
{
    uint32_t v;
    std::memcpy(&v, p, 4);
    return (v * 2654435761u) >> (32 - kHashBits);
}
uint32_t agree(const uint8_t *p, const uint8_t *q, uint32_t max_len)
{
    uint32_t k = 0;
    while (k < max_len && p[k] == q[k]) ++k;
    return k;
}
} // namespace

extern "C" {

// The links of chunk `chunk` as the kernel stores them: prev[r] for r counted from the window's start.  -> their number.
uint32_t emu_effort_links(const uint8_t *data, uint64_t len, uint64_t chunk, uint32_t substep, uint16_t *prev)
{
    const uint64_t c0 = chunk * kChunk, wstart = c0 > kWindow ? c0 - kWindow : 0;
    const uint32_t n = static_cast<uint32_t>(len - c0 < kChunk ? len - c0 : kChunk), wlen = static_cast<uint32_t>(c0 - wstart), total = wlen + n;
    std::vector<uint32_t> head(1u << kHashBits, 0), hv(substep);
    for (uint32_t sub = 0; sub < total; sub += substep) {
        const uint32_t end = sub + substep < total ? sub + substep : total;
        for (uint32_t r = sub; r < end; ++r) { // every look-up of the sub-step ...
            const uint64_t a = wstart + r;
            const bool hashed = r < wlen ? a + 4 <= len : r - wlen + 4 <= n;
            hv[r - sub] = hashed ? hash4(data + a) : 0xFFFF;
            prev[r] = static_cast<uint16_t>(hashed ? chain_link(r, head[hv[r - sub]]) : 0);
        }
        for (uint32_t r = sub; r < end; ++r) // ... before its inserts
            if (hv[r - sub] != 0xFFFF && head[hv[r - sub]] < r + 1) head[hv[r - sub]] = r + 1;
    }
    return total;
}

// The tokens of chunk `chunk`: out[i] = token, at[i] = its position in the chunk.  -> their number.
uint32_t emu_effort_tokens(const uint8_t *data, uint64_t len, uint64_t chunk, uint32_t bpp, uint32_t row, uint32_t substep, uint32_t probes,
                           uint32_t *out, uint32_t *at)
{
    const uint64_t c0 = chunk * kChunk, wstart = c0 > kWindow ? c0 - kWindow : 0;
    const uint32_t n = static_cast<uint32_t>(len - c0 < kChunk ? len - c0 : kChunk), wlen = static_cast<uint32_t>(c0 - wstart);
    std::vector<uint16_t> prev(kWindow + 65536);
    emu_effort_links(data, len, chunk, substep, prev.data());
    std::vector<uint32_t> best_len(n + 1, 0), best_dist(n + 1, 0);
    for (uint32_t p = 0; p < n; ++p) {
        const uint64_t a = c0 + p;
        const uint32_t max_len = n - p < kMaxMatch ? n - p : kMaxMatch;
        uint32_t bl = 0, bd = 0;
        auto attempt = [&](uint64_t d) {
            if (d == 0 || d > kWindow || d > a || bl == max_len) return;
            const uint32_t l = agree(data + a, data + a - d, max_len);
            if (l > bl || (l == bl && d < bd)) { bl = l; bd = static_cast<uint32_t>(d); }
        };
        if (max_len >= kMinMatch) {
            attempt(1);
            if (bpp > 1) attempt(bpp);
            uint32_t dist = 0;
            for (uint32_t k = 0; k < probes && bl < max_len; ++k) {
                dist = chain_step(dist, prev[wlen + p - dist]);
                if (!dist) break;
                attempt(dist);
            }
            if (row > 1 && row != bpp) attempt(row);
        }
        best_len[p] = kept_length(bl, bd);
        best_dist[p] = bd;
    }
    uint32_t count = 0;
    for (uint32_t p = 0; p < n;) { // (best_len[n] is 0: no next position in the chunk)
        const bool lit = !best_len[p] || lazy_defers(best_len[p], best_len[p + 1]);
        at[count] = p;
        out[count++] = lit ? data[c0 + p] : token_match(best_len[p], best_dist[p]);
        p = lazy_next(p, best_len[p], best_len[p + 1]);
    }
    return count;
}

uint32_t emu_chain_link(uint32_t pos, uint32_t head) { return chain_link(pos, head); }
uint32_t emu_chain_step(uint32_t dist, uint32_t link) { return chain_step(dist, link); }
uint32_t emu_kept_length(uint32_t len, uint32_t dist) { return kept_length(len, dist); }
uint32_t emu_lazy_next(uint32_t p, uint32_t len_here, uint32_t len_next) { return lazy_next(p, len_here, len_next); }

} // extern "C"
