// TEST HARNESS — the segment arithmetic of the PNG batch kernels (png_deflate_math.h) behind a C interface for ctypes.
#include "../../pixo_amd/csrc/png_deflate_math.h"

using namespace pixo_pngz;

extern "C" {

uint32_t emu_segment_bytes() { return sizeof(ZSegment); }
// lens[n] -> the table of n + 1 entries as seg_layout fills it in (src: the streams back to back); 0: refused
int emu_seg_layout(const uint64_t *lens, uint32_t n, ZSegment *table)
{
    uint64_t src = 0;
    for (uint32_t s = 0; s < n; ++s) { table[s] = ZSegment{src, lens[s], 0, 0, 0, 0, 0, 0, 0}; src += lens[s]; }
    return seg_layout(table, n) ? 1 : 0;
}
uint32_t emu_seg_of_chunk(const ZSegment *table, uint32_t n, uint32_t g) { return seg_of_chunk(table, n, g); }
uint32_t emu_seg_of_piece(const ZSegment *table, uint32_t n, uint32_t g) { return seg_of_piece(table, n, g); }
// out: c0, wstart, n, last
void emu_chunk_span(uint64_t len, uint64_t chunk, uint64_t out[4])
{
    const ChunkSpan s = chunk_span(len, chunk);
    out[0] = s.c0; out[1] = s.wstart; out[2] = s.n; out[3] = s.last ? 1 : 0;
}
uint32_t emu_piece_span(uint64_t stream_len, uint64_t piece, uint64_t *s0) { return piece_span(stream_len, piece, s0); }
uint64_t emu_seg_chunks(uint64_t len) { return seg_chunks(len); }
uint64_t emu_seg_pieces(uint64_t len) { return seg_pieces(len); }
uint64_t emu_seg_dst_bytes(uint64_t len) { return seg_dst_bytes(len); }
uint64_t emu_seg_framed_size(uint64_t stream_len) { return seg_framed_size(stream_len); }
uint64_t emu_seg_framed_offset(uint64_t s) { return seg_framed_offset(s); }
uint64_t emu_stored_bound(uint64_t len) { return stored_bound(len); }

} // extern "C"
