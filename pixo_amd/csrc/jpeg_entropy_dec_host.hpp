// jpeg_entropy_dec_host.hpp — the host's share of the device Huffman decode (PIXO_DECODE_DEVICE_ENTROPY): which files go to the
// device, and the record a file's workgroups read (jpeg_entropy_dec_math.h).  Plain C++, no HIP: the driver
// (jpeg_decode_api.cpp) and tests/emu_jpeg_entropy_dec compile the same code.
#pragma once
#include <cstring>

#include "jpeg_decode_host.hpp"
#include "jpeg_entropy_dec_math.h"

namespace pixo_jent {

// The host decodes from the start: files with a restart interval (the device form of those is a later request), files without
// MCUs, scans too short to be worth a record and scans whose bit positions would not fit 32 bits.
inline bool device_takes(const pixo_jdec_host::File &f)
{
    return f.restart == 0 && f.mcus_x != 0 && f.mcus_y != 0 && f.ecs_len >= kMinScanBytes && f.ecs_len < kMaxScanBytes;
}

inline void fill_table(const pixo_jdec_host::Huff &h, Table &t)
{
    for (int i = 0; i < 256; ++i) t.look[i] = static_cast<uint16_t>(h.look_len[i] ? (h.look_len[i] << 8) | h.look_sym[i] : 0);
    std::memcpy(t.maxcode, h.maxcode, sizeof t.maxcode);
    std::memcpy(t.valoff, h.valoff, sizeof t.valoff);
    std::memcpy(t.vals, h.vals, sizeof t.vals);
    t.reserved = 0;
}

// Everything of the record that the file alone decides; the driver adds ecs_at, coef_at (+ the image's place), first_sub,
// first_group and image.
inline void fill_record(const pixo_jdec_host::File &f, FileRecord &r)
{
    std::memset(&r, 0, sizeof r);
    uint32_t bim = 0;
    for (uint32_t c = 0; c < f.ncomp; ++c) {
        fill_table(f.dc[f.comp[c].td], r.tables[2 * c]);
        fill_table(f.ac[f.comp[c].ta], r.tables[2 * c + 1]);
        r.coef_at[c] = f.plane_at(c);
        r.blocks_w[c] = f.blocks_w(c);
        r.comp_blocks[c] = f.blocks_w(c) * f.blocks_h(c);
        r.blocks += r.comp_blocks[c];
        for (uint32_t by = 0; by < f.comp_v(c); ++by)
            for (uint32_t bx = 0; bx < f.comp_h(c); ++bx, ++bim) {
                r.bim_comp[bim] = static_cast<uint8_t>(c); r.bim_bx[bim] = static_cast<uint8_t>(bx); r.bim_by[bim] = static_cast<uint8_t>(by);
            }
    }
    r.blocks_per_mcu = bim; // 1, 3, 4 or 6: the walk admits no other sampling
    r.ecs_len = static_cast<uint32_t>(f.ecs_len);
    r.ncomp = f.ncomp;
    r.mcus_x = f.mcus_x;
    r.subs = subs_of(r.ecs_len);
    r.groups = groups_of(r.subs);
}

} // namespace pixo_jent
