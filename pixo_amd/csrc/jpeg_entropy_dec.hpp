// jpeg_entropy_dec.hpp — launchers of the device Huffman decode (jpeg_entropy_dec.hip; the arithmetic: jpeg_entropy_dec_math.h).
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_entropy_dec_math.h"

namespace pixo_dev {

// One sub-batch's device Huffman decode.  Everything is device memory; nothing is read before a launch has written it but
// `counters` and `status`, which the caller zeroes (and `coef`, zeroed before launch_jpeg_entropy_finish).
struct JpegEntropyArgs {
    const pixo_jent::FileRecord *records; // in launch order
    uint32_t files, groups, subs;         // of the sub-batch: records, workgroups, subsequences
    const uint8_t *scans;                 // 16-byte aligned; records[i].ecs_at from here
    pixo_jent::State *entry, *exit;       // per subsequence: the state its last decode began with / ended with
    uint32_t *count, *first_block;        // ... the blocks it completed; the scan ordinal of its first block
    pixo_jent::State *border[2];          // per workgroup: its last lane's exit, written in turn launch by launch
    uint32_t *counters;                   // per launch two words: workgroups that want another launch, the most rounds one took
    pixo_jent::FileStatus *status;        // per file
    int16_t *coef;                        // the sub-batch's coefficients
};
// Launch `launch` (0: the cold decode) of the hand-over.  cap: the rounds a file may use over all launches.
hipError_t launch_jpeg_entropy_sync(const JpegEntropyArgs &a, uint32_t launch, uint32_t cap, hipStream_t stream);
// Verify and place, write, DC: three launches.  Files the verify pass does not vouch for are left alone.
hipError_t launch_jpeg_entropy_finish(const JpegEntropyArgs &a, hipStream_t stream);

} // namespace pixo_dev
