// jpeg_entropy_dec_math.h — the Huffman decode of a baseline scan on the device (jpeg_entropy_dec.hip, PIXO_DECODE_DEVICE_ENTROPY):
// everything a lane computes, as host/device inline code.  Compiled for gfx950 by jpeg_entropy_dec.hip and for the HOST by the
// driver (jpeg_decode_api.cpp builds the records with it) and by tests/emu_jpeg_entropy_dec, which runs the passes lane by lane.
// No HIP headers in here.
//
// The scan is cut into subsequences of kSubBytes raw (still byte-stuffed) bytes; lane j of a file decodes the symbols that START
// in [j * kSubBytes, (j + 1) * kSubBytes) and hands its exit state — bit position, block of the MCU, zigzag index — to lane
// j + 1.  A lane that starts in a wrong state usually falls into step with the true decode after a few symbols (the code is
// self-synchronising), so the states are handed over until nothing changes.  A workgroup owns kGroupSubs subsequences and does
// its own rounds through LDS; the states at the workgroups' borders cross in further launches (no kernel waits for another
// workgroup).  The rounds of a file — per launch those of its slowest workgroup — are capped at kRoundCap: a file that has not
// settled by then is not vouched for.
//
// POSITIONS are bit positions in the RAW bytes, 32 bits wide: the driver sends scans of kMaxScanBytes and more to the host.  A
// position is canonical: its byte is never the 0x00 behind a 0xFF.  THE END OF THE DATA is the first 0xFF that is followed by
// anything but 0x00 (a marker, a fill byte, the last byte): behind it the reader hands out zero bits, as the host's does, and a
// block that used one of them is not counted; a state behind the end is DEAD.  The host's reader skips fill bytes (FF FF) — this
// one stops at them, which is the cautious side: whatever completes in front of them is the host's decode, what does not goes to
// the host.  A code no table holds, a DC category above 15 and an index past 63 do NOT make a state dead: they are routine in
// speculative decodes, and a lane that stopped at one could never fall into step.  They are FLAWS — the lane notes the first
// and decodes on (decode_sub) —, errors only where they survive into the verified chain, and then the host's to word.
//
// Bounds: a lane reads byte i only when i < limit, the smaller of the scan's length and the end of what the workgroup staged;
// every loop consumes at least one bit per turn and ends at the subsequence's last bit.  A symbol is at most 16 + 15 bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PIXO_JE_HD __host__ __device__ inline
#else
#define PIXO_JE_HD inline
#endif

namespace pixo_jent {

#if !defined(PIXO_JE_SUB_BYTES)
#define PIXO_JE_SUB_BYTES 128 // (tools/jpeg_entropy_rounds.py builds the host emulation with 64 and 256 as well, to compare)
#endif
constexpr uint32_t kSubBytes = PIXO_JE_SUB_BYTES; // S: raw bytes of a subsequence (profiles/jpeg_entropy_rounds.txt)
constexpr uint32_t kGroupSubs = 256;          // subsequences (lanes) of a workgroup
constexpr uint32_t kRoundCap = 132;           // hand-over rounds of one file at most: twice the largest count measured
constexpr uint32_t kMinScanBytes = 16;        // shorter scans: the host's from the start (a record is 5.6 KB)
constexpr uint32_t kMaxScanBytes = 1u << 28;  // this and longer: the host's (positions are 32 bits of bits)
constexpr uint32_t kSlackBytes = 16;          // staged in front of and behind a workgroup's span: a symbol that starts in the span ends in here
constexpr uint32_t kGroupBytes = kSubBytes * kGroupSubs;

// A Huffman table as the lanes read it: the host's Huff (jpeg_decode_host.hpp) with the two look-up arrays in one
struct Table {
    uint16_t look[256];  // length << 8 | symbol of the code of up to 8 bits the next 8 bits start with; 0: none
    int32_t maxcode[18]; // [l]: the largest code of length l, -1: none
    int32_t valoff[17];  // [l]: index of the first value of length l minus its code
    uint8_t vals[256];
    uint32_t reserved;
};
static_assert(sizeof(Table) == 912 && sizeof(Table) % 16 == 0, "tables are uploaded as they lie");

// What a workgroup needs of its file (uploaded as it lies, copied into LDS)
struct FileRecord {
    Table tables[6];       // [2 c] the DC table of component c, [2 c + 1] its AC table
    uint64_t ecs_at;       // bytes from the sub-batch's scans to this one (a multiple of 16; padded with zeros to one)
    uint64_t coef_at[3];   // bytes from the sub-batch's coefficients to each component's plane
    uint32_t ecs_len;
    uint32_t ncomp, mcus_x, blocks;  // blocks: of all components, the scan's
    uint32_t blocks_per_mcu;
    uint32_t blocks_w[3];  // blocks across a component's padded plane
    uint32_t comp_blocks[3]; // blocks of a component (the DC pass)
    uint32_t subs, first_sub;     // subsequences; the sub-batch's in front of this file's
    uint32_t groups, first_group; // workgroups; the launch's in front of this file's
    uint32_t image;        // the file's index in the call
    uint8_t bim_comp[8], bim_bx[8], bim_by[8]; // block of the MCU -> component, block across / down within the MCU
    uint32_t reserved[6];
};
static_assert(sizeof(FileRecord) == 5616 && sizeof(FileRecord) % 16 == 0, "records are uploaded as they lie");

// What the verify pass says of a file
enum Why { VOUCHED = 0, CHAIN_DEAD = 1, NOT_SETTLED = 2, SHORT = 3 }; // a dead state or a flawed lane in the chain; a lane not started from its predecessor's exit; the chain ends before the last block
struct FileStatus {
    uint32_t vouched, why, subs, rounds;
    uint32_t last_sub; // the subsequence that completes the last block (vouched)
    uint32_t used[2];  // the rounds the file has used, written in turn launch by launch (the sync kernel's)
    uint32_t reserved;
};

// ---- lane states ----------------------------------------------------------------------------------------------------------------
typedef uint64_t State; // bit position << 32 | block of the MCU << 8 | zigzag index (0: the DC code is next)
constexpr State kDead = ~uint64_t{0};
PIXO_JE_HD State make_state(uint32_t pos, uint32_t bim, uint32_t k) { return (uint64_t{pos} << 32) | (bim << 8) | k; }
PIXO_JE_HD uint32_t state_pos(State s) { return (uint32_t)(s >> 32); }
PIXO_JE_HD uint32_t state_bim(State s) { return ((uint32_t)s >> 8) & 0xFF; }
PIXO_JE_HD uint32_t state_k(State s) { return (uint32_t)s & 0xFF; }

PIXO_JE_HD uint32_t subs_of(uint32_t ecs_len) { return (ecs_len + kSubBytes - 1) / kSubBytes; }
PIXO_JE_HD uint32_t groups_of(uint32_t subs) { return (subs + kGroupSubs - 1) / kGroupSubs; }
// The bytes a workgroup stages: [lo, hi) of the scan (lo a multiple of 16; the scan is padded with zeros to one)
PIXO_JE_HD uint32_t stage_lo(uint32_t group) { return group ? group * kGroupBytes - kSlackBytes : 0u; }
PIXO_JE_HD uint32_t stage_hi(uint32_t group, uint32_t ecs_len)
{
    const uint64_t want = uint64_t{group + 1} * kGroupBytes + kSlackBytes, all = (uint64_t{ecs_len} + 15) & ~uint64_t{15};
    return (uint32_t)(want < all ? want : all);
}
// Where staged byte `rel` (from lo) lies in LDS: four bytes of padding per 128, so that lanes a subsequence apart hit different banks
PIXO_JE_HD uint32_t lds_at(uint32_t rel) { return rel + ((rel >> 7) << 2); }
constexpr uint32_t kStageBytes = kGroupBytes + 2 * kSlackBytes;
constexpr uint32_t kStageLds = kStageBytes + (kStageBytes >> 7) * 4 + 16;

// The file a workgroup belongs to: the last record with first_group <= g (records in launch order, none without workgroups)
template <class R> PIXO_JE_HD uint32_t file_of_group(const R *records, uint32_t count, uint32_t g)
{
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (records[mid].first_group <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the bit reader -------------------------------------------------------------------------------------------------------------
// Bytes: by(i) is raw byte i of the scan, asked only for i < limit.
template <class Bytes> struct Reader {
    const Bytes &by;
    uint32_t limit;   // no byte at or behind this index is read
    uint32_t end_idx; // the data ends in front of this raw index (limit until the end is seen)
    uint32_t pos;     // the next bit
    uint32_t idx[6];  // of the last window: raw index of the data byte k bytes behind the one `pos` is in
    PIXO_JE_HD Reader(const Bytes &b, uint32_t lim, uint32_t p) : by(b), limit(lim), end_idx(lim), pos(p) {}
    // The data byte at raw index i, and the index of the one behind it
    PIXO_JE_HD uint32_t data_byte(uint32_t i, uint32_t &next)
    {
        next = i + 1;
        if (i >= end_idx) return 0;
        const uint32_t b = by(i);
        if (b != 0xFF) return b;
        if (i + 1 < limit && by(i + 1) == 0x00) { next = i + 2; return 0xFF; }
        end_idx = i;
        return 0;
    }
    // The next 32 bits from `pos`, of which the first 25 at least are the scan's
    PIXO_JE_HD uint32_t window()
    {
        uint32_t i = pos >> 3, w = 0;
        idx[0] = i;
        for (int k = 0; k < 4; ++k) {
            uint32_t next;
            w = (w << 8) | data_byte(i, next);
            i = next;
            idx[k + 1] = i;
        }
        return w << (pos & 7);
    }
    // `n` (0..25) bits on, behind a window() from the same position
    PIXO_JE_HD void advance(uint32_t n)
    {
        const uint32_t bit = (pos & 7) + n;
        const uint32_t k = bit >> 3; // 0..4
        const uint32_t at = k == 0 ? idx[0] : k == 1 ? idx[1] : k == 2 ? idx[2] : k == 3 ? idx[3] : idx[4];
        pos = (at << 3) | (bit & 7);
    }
    PIXO_JE_HD bool overran() const { return pos > (end_idx << 3); } // a bit from behind the data was used
};

// The code the window starts with: its length (0: none of the table) and symbol
PIXO_JE_HD uint32_t decode_code(const Table &t, uint32_t w, uint32_t &sym)
{
    const uint32_t look = w >> 16;
    const uint32_t e = t.look[look >> 8];
    if (e) { sym = e & 0xFF; return e >> 8; }
    for (uint32_t l = 9; l <= 16; ++l) {
        const int32_t code = (int32_t)(look >> (16 - l));
        if (code <= t.maxcode[l]) {
            const int32_t at = t.valoff[l] + code;
            if (at < 0 || at > 255) return 0;
            sym = t.vals[at];
            return l;
        }
    }
    return 0;
}
PIXO_JE_HD int32_t extend(uint32_t v, uint32_t t) { return v >= (1u << (t - 1)) ? (int32_t)v : (int32_t)v - (int32_t)(1u << t) + 1; }

// Lane j's state before anyone has told it anything: the subsequence's first byte (the one behind it where that is the 0x00 of
// a stuffed pair), the MCU's first block, its DC code.  For lane 0 this is the true state.
template <class Bytes> PIXO_JE_HD State cold_entry(const Bytes &by, uint32_t limit, uint32_t j)
{
    uint32_t i = j * kSubBytes;
    if (j && i < limit && by(i) == 0x00 && by(i - 1) == 0xFF) ++i;
    return make_state(i << 3, 0, 0);
}

// What a lane's decode leaves behind
struct Exit {
    State state;     // at the first symbol boundary at or behind stop_bit, or kDead
    uint32_t blocks; // completed in front of the data's end
    uint32_t clean;  // ... in front of the first flaw as well (blocks, where there was none)
    uint32_t flawed; // 1: the lane met a code no table holds, a DC category above 15 or an index past 63
    PIXO_JE_HD uint32_t packed() const { return clean | (flawed << 31); } // what the kernels keep per lane (clean < 2^31)
};
struct NoSink {
    PIXO_JE_HD void block(uint32_t) {}
    PIXO_JE_HD void dc(int32_t) {}
    PIXO_JE_HD void ac(uint32_t, int32_t) {}
};

// Lane j from state `in`: symbol after symbol while the position is in front of stop_bit = (j + 1) * kSubBytes * 8, and while
// fewer than max_blocks blocks are complete (the write pass stops behind the file's last block).  sink.block(n): the n-th block
// this lane touches begins (or is resumed: n = 0 with in's zigzag index > 0); sink.dc / sink.ac: its values, ac's index in zigzag order.
// A FLAW — a code no table holds, a DC category above 15, an index past 63 — does not stop the lane: a lane that starts in a
// wrong state meets them all the time, and one that stopped there could never fall into step.  It skips a bit, or takes the
// category for 0, or ends the block, remembers how many blocks it had completed until then, and goes on.  A flawed lane in the
// verified chain in front of the last block is what the host refuses.
template <class Bytes, class Sink>
PIXO_JE_HD Exit decode_sub(const Bytes &by, uint32_t limit, const FileRecord &f, uint32_t j, State in, uint32_t max_blocks, Sink &sink)
{
    Exit x;
    x.state = kDead;
    x.blocks = x.clean = x.flawed = 0;
    const uint32_t start_bit = j * kSubBytes * 8, stop_bit = start_bit + kSubBytes * 8;
    if (in == kDead || max_blocks == 0) return x;
    uint32_t bim = state_bim(in), k = state_k(in);
    // (states are the kernels' own; one that is not a lane j entry state is treated as dead all the same)
    if (state_pos(in) < start_bit || state_pos(in) >= stop_bit + 8 * kSlackBytes || bim >= f.blocks_per_mcu || k > 63) return x;
    Reader<Bytes> r(by, limit, state_pos(in));
    sink.block(0);
    while (r.pos < stop_bit) {
        const Table &t = f.tables[2 * f.bim_comp[bim] + (k ? 1 : 0)];
        uint32_t w = r.window(), sym = 0;
        const uint32_t len = decode_code(t, w, sym);
        uint32_t size = 0, done = 0, flaw = 0; // done: the block is complete
        if (len == 0) {
            flaw = 1;
            r.advance(1);
        } else {
            if (k == 0) {
                size = sym;
                if (size > 15) { flaw = 1; size = 0; }
            } else {
                const uint32_t run = sym >> 4;
                size = sym & 15;
                if (size == 0) {
                    if (run != 15) done = 1;
                    else { k += 16; if (k > 64) { flaw = 1; done = 1; } }
                } else {
                    k += run;
                    if (k > 63) { flaw = 1; done = 1; size = 0; }
                }
            }
            uint32_t v = 0;
            if (len + size <= 25) {
                if (size) v = (w << len) >> (32 - size);
                r.advance(len + size);
            } else { // (a long code with many bits behind it: a second window)
                r.advance(len);
                w = r.window();
                v = w >> (32 - size);
                r.advance(size);
            }
            if (k == 0) {
                sink.dc(size ? extend(v, size) : 0);
                k = 1;
            } else if (size) {
                sink.ac(k, extend(v, size));
                ++k;
            }
        }
        if (flaw && !x.flawed) { x.flawed = 1; x.clean = x.blocks; }
        if (done || k >= 64) {
            if (r.overran()) break;
            ++x.blocks;
            bim = bim + 1 == f.blocks_per_mcu ? 0 : bim + 1;
            k = 0;
            if (x.blocks == max_blocks) break;
            sink.block(x.blocks);
        }
    }
    if (!x.flawed) x.clean = x.blocks;
    if (!r.overran()) x.state = make_state(r.pos, bim, k);
    return x;
}

// ---- where a block's coefficients go ----------------------------------------------------------------------------------------------
// Block `ordinal` of the scan (< f.blocks): its component and its raster index in the component's padded plane
PIXO_JE_HD void place_block(const FileRecord &f, uint32_t ordinal, uint32_t &comp, uint64_t &raster)
{
    const uint32_t mcu = ordinal / f.blocks_per_mcu, bim = ordinal - mcu * f.blocks_per_mcu;
    const uint32_t my = mcu / f.mcus_x, mx = mcu - my * f.mcus_x;
    comp = f.bim_comp[bim];
    const uint32_t h = comp == 0 && f.ncomp == 3 ? f.blocks_w[0] / f.mcus_x : 1u, v = comp == 0 ? f.blocks_per_mcu == 6 ? 2u : 1u : 1u;
    raster = (uint64_t{my} * v + f.bim_by[bim]) * f.blocks_w[comp] + (uint64_t{mx} * h + f.bim_bx[bim]);
}
// The n-th block of component c in scan order (the DC pass): its raster index
PIXO_JE_HD uint64_t scan_order_block(const FileRecord &f, uint32_t c, uint32_t n)
{
    const uint32_t h = c == 0 && f.ncomp == 3 ? f.blocks_w[0] / f.mcus_x : 1u, v = c == 0 && f.blocks_per_mcu == 6 ? 2u : 1u;
    const uint32_t per = h * v, mcu = n / per, r = n - mcu * per;
    const uint32_t my = mcu / f.mcus_x, mx = mcu - my * f.mcus_x;
    return (uint64_t{my} * v + r / h) * f.blocks_w[c] + (uint64_t{mx} * h + r % h);
}
// (jpeg_decode_math.h coef_index, restated so that this header stands alone; a static_assert in the kernel file compares them)
PIXO_JE_HD constexpr uint64_t coef_index(uint64_t block, uint32_t natural) { return (block >> 6) * 4096 + (natural >> 3) * 512 + (block & 63) * 8 + (natural & 7); }

// The sink of the write pass: non-zero ACs to their places, each block's DC DIFFERENCE to position 0 (the DC pass sums them).
// first: the scan ordinal of the lane's first block; blocks at and behind f.blocks are never begun (max_blocks).
struct WriteSink {
    const FileRecord &f;
    int16_t *coef; // the sub-batch's coefficients
    const uint8_t *zigzag;
    uint32_t first;
    int16_t *at;
    PIXO_JE_HD WriteSink(const FileRecord &file, int16_t *c, const uint8_t *z, uint32_t first_block) : f(file), coef(c), zigzag(z), first(first_block), at(nullptr) {}
    PIXO_JE_HD void block(uint32_t n)
    {
        uint32_t comp;
        uint64_t raster;
        place_block(f, first + n, comp, raster);
        at = coef + f.coef_at[comp] / 2 + coef_index(raster, 0);
    }
    PIXO_JE_HD void dc(int32_t diff) { at[0] = (int16_t)diff; }
    PIXO_JE_HD void ac(uint32_t k, int32_t v)
    {
        const uint32_t natural = zigzag[k];
        at[(natural >> 3) * 512 + (natural & 7)] = (int16_t)v;
    }
};

} // namespace pixo_jent
