// TEST HARNESS — shared by the shim and the stand-alone fuzz program: one zlib stream through the host build of the device walk.
#pragma once
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../../pixo_amd/csrc/png_inflate_math.h"

// data[2, len - 4) is copied to an aligned block with 16 zero bytes behind it, as the driver stages it
inline uint32_t emu_inflate(const uint8_t *data, uint64_t len, uint8_t *out, uint64_t expected, uint64_t *produced, uint32_t *adler, uint64_t *turns,
                            uint64_t *bound)
{
    const uint64_t in_len = len >= 6 ? len - 6 : 0;
    std::vector<uint64_t> block((in_len + 16 + 15) / 8 + 2, 0); // (8-byte aligned storage; the walk needs 4)
    if (in_len) std::memcpy(block.data(), data + 2, in_len);
    std::unique_ptr<pixo_pngi::Shared> sh(new pixo_pngi::Shared());
    pixo_pngi::Walk w(*sh, reinterpret_cast<const uint8_t *>(block.data()), in_len, out, expected);
    const pixo_pngi::Result r = w.run();
    *produced = r.produced;
    *adler = r.adler;
    *turns = w.turns;
    *bound = 8 * in_len + expected + 1;
    return r.verdict;
}
