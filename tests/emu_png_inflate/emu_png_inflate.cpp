// TEST HARNESS — the device inflate's walk (pixo_amd/csrc/png_inflate_math.h) compiled for the host: every PNGI_LANES region
// runs lane 0..63 in turn, everything else once.  emu_pngi_inflate walks a whole zlib stream as a workgroup of the kernel does;
// emu_pngi_step replays one step of tokens lane by lane; the small entries expose the header's pieces.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "emu_png_inflate.hpp"

using namespace pixo_pngi;

extern "C" uint32_t emu_pngi_step_tokens(void) { return kStepTokens; }
extern "C" uint32_t emu_pngi_window_bytes(void) { return kWindowBytes; }
extern "C" uint32_t emu_pngi_far_distance(void) { return kFarDistance; }
extern "C" uint32_t emu_pngi_stored_chunk(void) { return kStoredChunk; }
extern "C" uint32_t emu_pngi_length_base(uint32_t c, uint32_t *extra) { return length_base(c, extra); }
extern "C" uint32_t emu_pngi_distance_base(uint32_t d, uint32_t *extra) { return distance_base(d, extra); }
extern "C" uint32_t emu_pngi_match_source(uint32_t i, uint32_t distance) { return match_source(i, distance); }
extern "C" uint32_t emu_pngi_code_length_order(uint32_t i) { return Walk::code_length_order(i); }

// zlib stream data[0, len) -> out[0, expected); the header's 2 bytes and the checksum's 4 are skipped, not checked (len >= 6).
// Returns the verdict; *turns: loop turns taken, *bound: what the header promises.
extern "C" uint32_t emu_pngi_inflate(const uint8_t *data, uint64_t len, uint8_t *out, uint64_t expected, uint64_t *produced, uint32_t *adler,
                                     uint64_t *turns, uint64_t *bound)
{
    return emu_inflate(data, len, out, expected, produced, adler, turns, bound);
}

// lengths[0, symbols) -> 0: the set is decodable and lut (1 << 10 entries of symbol | length << 12) is filled; 1: over-subscribed
extern "C" uint32_t emu_pngi_build(const uint8_t *lengths, uint32_t symbols, uint16_t *lut)
{
    std::unique_ptr<Shared> sh(new Shared());
    std::memcpy(sh->lengths, lengths, symbols);
    Walk w(*sh, nullptr, 0, nullptr, 0);
    if (!w.build(sh->lit, 0, symbols)) return 1;
    std::memcpy(lut, sh->lit.lut, sizeof sh->lit.lut);
    return 0;
}
// ... and the symbol | length << 12 the walk's decode finds for the 15 bits `bits` (0: none)
extern "C" uint32_t emu_pngi_decode(const uint8_t *lengths, uint32_t symbols, uint32_t bits)
{
    std::unique_ptr<Shared> sh(new Shared());
    std::memcpy(sh->lengths, lengths, symbols);
    alignas(16) uint32_t in[2] = {bits, 0};
    Walk w(*sh, reinterpret_cast<const uint8_t *>(in), 8, nullptr, 0);
    if (!w.build(sh->lit, 0, symbols)) return 0;
    uint32_t sym = 0;
    if (!w.decode(sh->lit, &sym)) return 0;
    return sym | (static_cast<uint32_t>(w.used) << 12);
}

// One step replayed lane by lane: `prefix` is the output so far (at most a window of it matters), tokens[0, count) as
// token_literal / token_match make them.  out receives the step's bytes; returns how many.
extern "C" uint64_t emu_pngi_step(const uint8_t *prefix, uint64_t prefix_len, const uint32_t *tokens, uint32_t count, uint8_t *out)
{
    std::unique_ptr<Shared> sh(new Shared());
    std::vector<uint8_t> sink(prefix_len + uint64_t{count} * kMaxMatch + 16);
    Walk w(*sh, nullptr, 0, sink.data(), sink.size());
    for (uint64_t i = 0; i < prefix_len; ++i) sh->ring[i & (kWindowBytes - 1)] = prefix[i];
    w.n = w.done = prefix_len;
    w.flushed = prefix_len & ~uint64_t{kFlushPiece - 1};
    for (uint32_t k = 0; k < count && k < kStepTokens; ++k) {
        sh->tok[k][0] = tokens[k];
        sh->tok[k][1] = static_cast<uint32_t>(w.n);
        if (token_length(tokens[k]) > 1) w.match_mask |= uint64_t{1} << k;
        w.n += token_length(tokens[k]);
        ++w.ntok;
    }
    w.run_step();
    const uint64_t made = w.done - prefix_len;
    for (uint64_t i = 0; i < made; ++i) out[i] = sh->ring[(prefix_len + i) & (kWindowBytes - 1)];
    return made;
}
