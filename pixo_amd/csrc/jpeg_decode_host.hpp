// jpeg_decode_host.hpp — the host side of JPEG decode (jpeg_decode_host.cpp): the marker walk and the entropy decoder.  Plain
// C++, no HIP: the library's driver (jpeg_decode_api.cpp) and the stand-alone sanitizer program of tests/emu_jpeg_decode
// compile the same file.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace pixo_jdec_host {

enum Kind { OK = 0, INVALID = 1, UNSUPPORTED = 2 }; // PIXO_OK, PIXO_ERR_INVALID_DECODE, PIXO_ERR_UNSUPPORTED_DECODE

// A Huffman table as the decoder reads it: codes of up to 8 bits by a look-up of the next 8 bits, longer ones canonically.
struct Huff {
    bool defined = false;
    uint8_t look_len[256]; // 0: the next 8 bits start no code of up to 8 bits
    uint8_t look_sym[256];
    int32_t maxcode[18];   // [l]: the largest code of length l, -1: none; [17]: a sentinel above every code
    int32_t valoff[17];    // [l]: index of the first value of length l minus its code
    uint8_t vals[256];
};
struct Component { uint8_t id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0; };

// What the walk found up to and including SOS
struct File {
    uint32_t width = 0, height = 0, ncomp = 0;
    int cls = 0; // pixo_jdec::C_GRAY .. C_420
    Component comp[3];
    uint16_t q[4][64]; // natural order
    bool q_defined[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    uint32_t restart = 0;
    const uint8_t *ecs = nullptr; // the entropy-coded segment: from behind SOS to the end of the file
    size_t ecs_len = 0;
    uint32_t mcus_x = 0, mcus_y = 0;

    uint32_t comp_h(uint32_t c) const { return ncomp == 1 ? 1u : comp[c].h; } // (a lone component's factors are ignored)
    uint32_t comp_v(uint32_t c) const { return ncomp == 1 ? 1u : comp[c].v; }
    uint32_t blocks_w(uint32_t c) const { return mcus_x * comp_h(c); }
    uint32_t blocks_h(uint32_t c) const { return mcus_y * comp_v(c); }
    uint64_t plane_blocks(uint32_t c) const { return (static_cast<uint64_t>(blocks_w(c)) * blocks_h(c) + 63) & ~uint64_t{63}; } // rounded up to 64
    uint64_t plane_at(uint32_t c) const // bytes from the image's coefficients to component c's plane
    {
        uint64_t at = 0;
        for (uint32_t k = 0; k < c; ++k) at += plane_blocks(k) * 128;
        return at;
    }
    uint64_t coef_bytes() const { return plane_at(ncomp); }
    uint8_t color_type() const { return ncomp == 1 ? 0 : 2; } // PIXO_GRAY, PIXO_RGB
    uint64_t pixel_bytes() const { return static_cast<uint64_t>(width) * height * (ncomp == 1 ? 1 : 3); }
};

// The walk from SOI to SOS with its checks, in the order jpeg_decode_api.cpp's head comment gives.  *msg: the refusal's text
// without its "Decode error: " / "Unsupported: " prefix.
Kind walk(const uint8_t *data, size_t len, File &f, std::string *msg);
// The scan -> the quantised coefficients of every component, in the layout of jpeg_decode_math.h, at `coef` (f.coef_bytes()
// bytes, zeroed here first).  Refuses a scan that breaks off, a code no table holds, a coefficient index past 63 and a missing
// or out-of-sequence restart marker; never reads outside [f.ecs, f.ecs + f.ecs_len) nor writes outside the planes.
Kind entropy_decode(const File &f, int16_t *coef, std::string *msg);

extern const uint8_t kZigzag[64]; // zigzag index -> natural index

} // namespace pixo_jdec_host
