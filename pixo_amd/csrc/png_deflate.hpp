// png_deflate.hpp — host-callable launchers of the device DEFLATE (png_deflate.hip): one or more runs of bytes in HBM -> a
// zlib stream each in HBM, optionally laid out as the bodies of 256 KiB IDAT chunks with room for their frames, and the
// CRC-32 of their pieces.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "png_deflate_math.h"

namespace pixo_dev {

constexpr uint32_t kZChunk = 65535;       // input bytes per DEFLATE block: a stored block's LEN is 16 bits
constexpr uint32_t kZSlot = 65552;        // bytes of a block's slot (chunk + 5 for the stored form, rounded up to 16)
constexpr uint32_t kZTokStride = 65536;   // u32 tokens per chunk in the token scratch
constexpr uint32_t kIdatBytes = 256 * 1024; // src/png/mod.rs:621
constexpr uint32_t kCrcPiece = 4096;      // bytes of the stream one CRC value covers (divides kIdatBytes)
// The high effort ("the second finder"): positions whose look-ups come before their inserts, and the
// entries of a hash chain tried at a position.  Chosen on the MI355X from {64, 256} x {4, 8} (profiles/png_encode_timing.txt).
#ifndef PIXO_PNG_EFFORT_SUBSTEP
#define PIXO_PNG_EFFORT_SUBSTEP 64
#endif
#ifndef PIXO_PNG_EFFORT_PROBES
#define PIXO_PNG_EFFORT_PROBES 8
#endif
constexpr uint32_t kZEffortSubstep = PIXO_PNG_EFFORT_SUBSTEP, kZEffortProbes = PIXO_PNG_EFFORT_PROBES;
constexpr uint32_t kZPrevStride = 32768 + 65536; // u16 links per chunk in the link scratch: its window, then the chunk
static_assert(kZEffortSubstep % 64 == 0 && 32768 % kZEffortSubstep == 0, "whole wavefronts; the window is whole sub-steps");

struct ZChunkInfo {
    uint32_t bytes; // of the block in its slot, the trailing empty stored block included
    uint32_t mode;  // 0 stored, 1 fixed, 2 dynamic
    unsigned long long sum_a, sum_b; // Adler-32 partial sums of the chunk: sum of bytes, sum of (n - i) * byte_i
};

inline uint64_t z_chunks(uint64_t len) { return (len + kZChunk - 1) / kZChunk; }
// Where byte s of the zlib stream lies in a destination: framed = the body of IDAT chunk s / 256 KiB, each chunk
// preceded by 8 bytes (length, type) and followed by 4 (CRC).
inline uint64_t z_framed_size(uint64_t stream_len) { return stream_len + 12 * ((stream_len + kIdatBytes - 1) / kIdatBytes); }

// A launch works on nseg streams (segments, png_deflate_math.h ZSegment) at once; a single stream is a table of one.
// d_segs: the table of nseg + 1 entries that seg_layout filled in, in device memory; d_data / d_dst: what the segments' src
// / dst count from.  The scratch is indexed by global chunk (`chunks` = d_segs[nseg].first_chunk of them): d_tok: chunks *
// kZTokStride u32; d_slots: chunks * kZSlot bytes; d_info: chunks entries.
static_assert(pixo_pngz::kSegChunk == kZChunk && pixo_pngz::kSegIdat == kIdatBytes && pixo_pngz::kSegPiece == kCrcPiece, "one set of sizes");
static_assert(sizeof(pixo_pngz::ZSegment) == 48, "the table's layout is the same on both sides");
static_assert(kCrcPiece % 4 == 0 && kIdatBytes % kCrcPiece == 0, "a CRC piece starts on a word of the framed stream and lies inside one IDAT chunk");
// One workgroup per chunk of every segment: match finding, parse, Huffman codes, the smallest of stored / fixed / dynamic into
// the chunk's slot; no chunk looks in front of its segment's first byte.  The segment's hint_bpp / hint_row: distances tried
// at every position besides 1 and the hash table's (0 or out of range: not tried).
// effort 0: the table's latest occurrence, greedy parse (d_prev is not read).  effort 1: hash chains of kZEffortProbes entries
// linked in sub-steps of kZEffortSubstep, one-step lazy parse; d_prev: chunks * kZPrevStride u16.
hipError_t launch_deflate(const void *d_data, const pixo_pngz::ZSegment *d_segs, uint32_t nseg, uint32_t chunks, uint32_t effort, uint32_t *d_tok,
                          uint16_t *d_prev, uint8_t *d_slots, ZChunkInfo *d_info, hipStream_t stream);
// Scan (d_offsets: `chunks` u64, restarting at every segment; d_totals: nseg u64, each segment's block bytes), compaction
// (every segment's header, blocks and d_segs[s].adler at d_dst + dst) and, where d_crc is given, the CRC-32 of every 4 KiB
// piece (d_crc: `pieces` = d_segs[nseg].first_piece words; segment s's values start at first_piece, those behind its
// stream's end are not written).  framed: the streams as IDAT bodies with room for their frames, d_dst 16-byte aligned (the
// launch is refused otherwise); unframed: the bare stream at any address, bytes where words would not be aligned, no CRC.
// d_segs[s].adler must be final by now.
hipError_t launch_deflate_finish(const uint8_t *d_slots, const ZChunkInfo *d_info, const pixo_pngz::ZSegment *d_segs, uint32_t nseg, uint32_t chunks,
                                 uint32_t pieces, uint32_t header, unsigned long long *d_offsets, unsigned long long *d_totals, uint8_t *d_dst,
                                 bool framed, uint32_t *d_crc, hipStream_t stream);

} // namespace pixo_dev
