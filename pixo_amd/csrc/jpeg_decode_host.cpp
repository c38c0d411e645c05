// jpeg_decode_host.cpp — the host side of JPEG decode: the marker walk (pixo::decode::decode_jpeg, reference
// src/decode/jpeg.rs:214-484, restated in its order and with its messages) and an entropy decoder of our own — Huffman codes of
// up to 8 bits by a look-up of the next 8 bits, longer ones canonically; restart intervals by the standard: the padding is
// discarded, the marker's number checked, the predictors reset.  The quantised coefficients go straight into the layout the
// kernel loads (jpeg_decode_math.h).  The bytes are untrusted: every read is bounded by the file's length, every write by the
// planes' sizes; tests/emu_jpeg_decode runs this file under the host sanitizers over mutated files.
//
// Two departures from the reference, on purpose: a scan that breaks off is refused — the reference returns the
// part it has decoded —, and a restart marker that sits where the reference's bit reader drops unconsumed bits decodes correctly.
#include "jpeg_decode_host.hpp"

#include <cstring>

#include "jpeg_decode_math.h"

namespace pixo_jdec_host {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

namespace {

Kind refuse(Kind k, std::string *msg, const std::string &text)
{
    if (msg) *msg = text;
    return k;
}
uint32_t be16(const uint8_t *p) { return (uint32_t{p[0]} << 8) | p[1]; }

// BITS and HUFFVAL -> the decoder's table.  false: the lengths describe no prefix code (more codes of a length than it has).
bool build_huff(const uint8_t bits[16], const uint8_t *vals, size_t n, Huff &h)
{
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.vals, vals, n);
    uint32_t code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        h.valoff[l] = static_cast<int32_t>(k) - static_cast<int32_t>(code);
        if (bits[l - 1]) {
            if (code + bits[l - 1] > (1u << l)) return false;
            for (uint32_t i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
                if (l > 8) continue;
                for (uint32_t fill = 0; fill < (1u << (8 - l)); ++fill) { // every 8-bit window that starts with this code
                    h.look_len[(code << (8 - l)) | fill] = static_cast<uint8_t>(l);
                    h.look_sym[(code << (8 - l)) | fill] = vals[k];
                }
            }
            h.maxcode[l] = static_cast<int32_t>(code) - 1;
        } else {
            h.maxcode[l] = -1;
        }
        code <<= 1;
    }
    h.maxcode[17] = 0x7FFFFFFF;
    h.defined = true;
    return true;
}

} // namespace

Kind walk(const uint8_t *d, size_t len, File &f, std::string *msg)
{
    if (len < 2 || d[0] != 0xFF || d[1] != 0xD8) return refuse(INVALID, msg, "not a JPEG file");
    size_t pos = 2;
    bool adobe = false;
    uint8_t adobe_transform = 0;
    for (;;) {
        // read_marker (jpeg.rs:253-292): to the next 0xFF, over the fill bytes, the marker, its segment
        while (pos < len && d[pos] != 0xFF) ++pos;
        while (pos < len && d[pos] == 0xFF) ++pos;
        if (pos >= len) return refuse(INVALID, msg, "unexpected end of file");
        const uint8_t marker = d[pos++];
        const uint8_t *seg = nullptr;
        size_t n = 0;
        if (!(marker == 0xD8 || marker == 0xD9 || (marker >= 0xD0 && marker <= 0xD7))) {
            if (pos + 2 > len) return refuse(INVALID, msg, "truncated marker");
            const size_t length = be16(d + pos);
            pos += 2;
            if (length < 2 || pos + length - 2 > len) return refuse(INVALID, msg, "invalid marker length");
            seg = d + pos;
            n = length - 2;
            pos += n;
        }
        if (marker == 0xC0) { // SOF0
            if (n < 8) return refuse(INVALID, msg, "invalid SOF0 length");
            if (seg[0] != 8) return refuse(UNSUPPORTED, msg, std::to_string(seg[0]) + "-bit precision not supported");
            f.height = be16(seg + 1);
            f.width = be16(seg + 3);
            const uint32_t nc = seg[5];
            if (nc != 1 && nc != 3) return refuse(UNSUPPORTED, msg, std::to_string(nc) + " components not supported");
            if (n < 6 + nc * 3) return refuse(INVALID, msg, "truncated SOF0 components");
            f.ncomp = 0;
            for (uint32_t i = 0; i < nc; ++i) {
                const uint8_t *c = seg + 6 + 3 * i;
                const uint32_t h = c[1] >> 4, v = c[1] & 15;
                if (h == 0 || v == 0)
                    return refuse(INVALID, msg, "invalid sampling factors " + std::to_string(h) + "x" + std::to_string(v) + " for component " + std::to_string(c[0]));
                if (c[2] > 3) return refuse(INVALID, msg, "invalid quantization table ID " + std::to_string(c[2]) + " for component " + std::to_string(c[0]));
                f.comp[i].id = c[0]; f.comp[i].h = static_cast<uint8_t>(h); f.comp[i].v = static_cast<uint8_t>(v); f.comp[i].tq = c[2];
            }
            f.ncomp = nc;
        } else if (marker == 0xC2) {
            return refuse(UNSUPPORTED, msg, "progressive JPEG not supported");
        } else if (marker == 0xC4) { // DHT
            size_t o = 0;
            while (o < n) {
                const uint8_t info = seg[o];
                if ((info & 15) > 3) return refuse(INVALID, msg, "invalid Huffman table ID");
                ++o;
                if (o + 16 > n) return refuse(INVALID, msg, "truncated DHT");
                const uint8_t *bits = seg + o;
                o += 16;
                size_t values = 0;
                for (int i = 0; i < 16; ++i) values += bits[i];
                if (o + values > n) return refuse(INVALID, msg, "truncated DHT values");
                // (ours: the reference builds whatever it is given)
                if (values > 256 || !build_huff(bits, seg + o, values, (info >> 4) == 0 ? f.dc[info & 15] : f.ac[info & 15]))
                    return refuse(INVALID, msg, "invalid Huffman code lengths");
                o += values;
            }
        } else if (marker == 0xDB) { // DQT: zigzag order in the file, natural order here
            size_t o = 0;
            while (o < n) {
                const uint8_t info = seg[o];
                const uint32_t id = info & 15;
                if (id > 3) return refuse(INVALID, msg, "invalid quantization table ID");
                ++o;
                const size_t bytes = (info >> 4) == 0 ? 64 : 128;
                if (o + bytes > n) return refuse(INVALID, msg, "truncated DQT");
                for (int i = 0; i < 64; ++i) f.q[id][kZigzag[i]] = static_cast<uint16_t>(bytes == 64 ? seg[o + i] : be16(seg + o + 2 * i));
                f.q_defined[id] = true;
                o += bytes;
            }
        } else if (marker == 0xDD) { // DRI
            if (n != 2) return refuse(INVALID, msg, "invalid DRI length");
            f.restart = be16(seg);
        } else if (marker == 0xEE) { // APP14: "Adobe", version, flags0, flags1, transform
            if (n >= 12 && !std::memcmp(seg, "Adobe", 5)) { adobe = true; adobe_transform = seg[11]; }
        } else if (marker == 0xDA) { // SOS
            if (n == 0) return refuse(INVALID, msg, "empty SOS segment");
            const uint32_t ns = seg[0];
            if (ns != f.ncomp) return refuse(INVALID, msg, "SOS component count mismatch");
            uint8_t scan_id[3] = {0, 0, 0};
            for (uint32_t i = 0; i < ns; ++i) {
                const size_t o = 1 + 2 * i;
                if (o + 1 >= n) return refuse(INVALID, msg, "truncated SOS segment");
                const uint32_t td = seg[o + 1] >> 4, ta = seg[o + 1] & 15;
                if (td > 3) return refuse(INVALID, msg, "invalid DC Huffman table ID " + std::to_string(td) + " for component " + std::to_string(seg[o]));
                if (ta > 3) return refuse(INVALID, msg, "invalid AC Huffman table ID " + std::to_string(ta) + " for component " + std::to_string(seg[o]));
                scan_id[i] = seg[o];
                f.comp[i].td = static_cast<uint8_t>(td); f.comp[i].ta = static_cast<uint8_t>(ta);
            }
            // ---- from here on the checks are ours ----
            if (f.ncomp == 0) return refuse(INVALID, msg, "SOS before SOF0");
            if (f.ncomp == 1) {
                f.cls = pixo_jdec::C_GRAY;
            } else {
                const Component *c = f.comp;
                const bool chroma_1x1 = c[1].h == 1 && c[1].v == 1 && c[2].h == 1 && c[2].v == 1;
                if (chroma_1x1 && c[0].h == 1 && c[0].v == 1) f.cls = pixo_jdec::C_444;
                else if (chroma_1x1 && c[0].h == 2 && c[0].v == 1) f.cls = pixo_jdec::C_422;
                else if (chroma_1x1 && c[0].h == 2 && c[0].v == 2) f.cls = pixo_jdec::C_420;
                else {
                    std::string s;
                    for (uint32_t i = 0; i < 3; ++i) s += (i ? " " : "") + std::to_string(c[i].h) + "x" + std::to_string(c[i].v);
                    return refuse(UNSUPPORTED, msg, "sampling factors " + s + " not supported");
                }
            }
            for (uint32_t i = 0; i < ns; ++i)
                if (scan_id[i] != f.comp[i].id) return refuse(UNSUPPORTED, msg, "a scan that does not hold all components in frame order is not supported");
            if (f.ncomp == 3 && adobe && adobe_transform != 1)
                return refuse(UNSUPPORTED, msg, "Adobe colour transform " + std::to_string(adobe_transform) + " not supported");
            if (f.ncomp == 3 && f.comp[0].id == 'R' && f.comp[1].id == 'G' && f.comp[2].id == 'B')
                return refuse(UNSUPPORTED, msg, "RGB component ids not supported");
            for (uint32_t i = 0; i < f.ncomp; ++i) {
                if (!f.q_defined[f.comp[i].tq]) return refuse(INVALID, msg, "quantization table " + std::to_string(f.comp[i].tq) + " is not defined");
                if (!f.dc[f.comp[i].td].defined) return refuse(INVALID, msg, "DC Huffman table " + std::to_string(f.comp[i].td) + " is not defined");
                if (!f.ac[f.comp[i].ta].defined) return refuse(INVALID, msg, "AC Huffman table " + std::to_string(f.comp[i].ta) + " is not defined");
            }
            f.mcus_x = (f.width + 8 * pixo_jdec::luma_h(f.cls) - 1) / (8 * pixo_jdec::luma_h(f.cls));
            f.mcus_y = (f.height + 8 * pixo_jdec::luma_v(f.cls) - 1) / (8 * pixo_jdec::luma_v(f.cls));
            f.ecs = d + pos;
            f.ecs_len = len - pos;
            // A block is at least two bits (a DC code and an end of block): a scan too short for the frame's blocks is refused
            // here, before anyone reserves 128 bytes per block for it.
            uint64_t blocks = 0;
            for (uint32_t i = 0; i < f.ncomp; ++i) blocks += static_cast<uint64_t>(f.blocks_w(i)) * f.blocks_h(i);
            if (blocks > static_cast<uint64_t>(f.ecs_len) * 4) return refuse(INVALID, msg, "entropy-coded segment ends early");
            return OK;
        } else if (marker == 0xD9) {
            break;
        } // everything else is skipped
    }
    return refuse(INVALID, msg, "no image data found");
}

namespace {

// The scan's bits, most significant first.  Stuffed 0xFF00 gives 0xFF; a marker stops the reader in front of it: from there
// on it hands out zero bits and counts them, and a block that used one of them is a scan that broke off.
struct BitReader {
    const uint8_t *p, *end;
    uint64_t buf = 0; // the next bits at the top
    int bits = 0;     // how many of them
    int fake = 0;     // ... of which at the tail: zeros from behind the data
    BitReader(const uint8_t *data, size_t n) : p(data), end(data + n) {}
    void fill()
    {
        while (bits <= 56) {
            uint64_t byte = 0;
            if (fake == 0 && p < end) {
                if (*p != 0xFF) byte = *p++;
                else if (p + 1 < end && p[1] == 0x00) { byte = 0xFF; p += 2; }
                else if (p + 1 < end && p[1] == 0xFF) { ++p; continue; } // a fill byte in front of a marker
                else fake = 8; // a marker, or the file's last byte
            } else {
                fake += 8;
            }
            buf |= byte << (56 - bits);
            bits += 8;
        }
    }
    uint32_t peek16() { if (bits < 16) fill(); return static_cast<uint32_t>(buf >> 48); }
    void drop(int n) { buf <<= n; bits -= n; }
    uint32_t take(int n) // 1..16
    {
        if (bits < n) fill();
        const uint32_t v = static_cast<uint32_t>(buf >> (64 - n));
        drop(n);
        return v;
    }
    bool overran() const { return fake > bits; }
    // At a restart: the rest of the last byte is padding; then fill bytes, then RSTn with n == expected
    bool restart(uint32_t expected)
    {
        if (overran()) return false;
        buf = 0; bits = 0; fake = 0;
        while (p + 1 < end && p[0] == 0xFF && p[1] == 0xFF) ++p;
        if (!(p + 1 < end && p[0] == 0xFF && p[1] == 0xD0 + (expected & 7))) return false;
        p += 2;
        return true;
    }
};

// -1: the next 16 bits start no code of the table
int decode_symbol(BitReader &br, const Huff &h)
{
    const uint32_t look = br.peek16();
    const uint32_t l8 = h.look_len[look >> 8];
    if (l8) { br.drop(static_cast<int>(l8)); return h.look_sym[look >> 8]; }
    for (int l = 9; l <= 16; ++l) {
        const int32_t code = static_cast<int32_t>(look >> (16 - l));
        if (code <= h.maxcode[l]) {
            const int32_t at = h.valoff[l] + code;
            if (at < 0 || at > 255) return -1;
            br.drop(l);
            return h.vals[at];
        }
    }
    return -1;
}
int32_t extend(uint32_t v, int t) { return v >= (1u << (t - 1)) ? static_cast<int32_t>(v) : static_cast<int32_t>(v) - (1 << t) + 1; }

} // namespace

Kind entropy_decode(const File &f, int16_t *coef, std::string *msg)
{
    if (f.coef_bytes()) std::memset(coef, 0, static_cast<size_t>(f.coef_bytes()));
    BitReader br(f.ecs, f.ecs_len);
    uint32_t pred[3] = {0, 0, 0}; // (unsigned: a hostile file may wrap it)
    int16_t *plane[3];
    for (uint32_t c = 0; c < f.ncomp; ++c) plane[c] = coef + f.plane_at(c) / 2;
    uint64_t mcu = 0;
    uint32_t next_rst = 0;
    for (uint32_t my = 0; my < f.mcus_y; ++my) {
        for (uint32_t mx = 0; mx < f.mcus_x; ++mx, ++mcu) {
            if (f.restart && mcu && mcu % f.restart == 0) {
                if (!br.restart(next_rst++)) return refuse(INVALID, msg, br.overran() ? "entropy-coded segment ends early" : "missing or out-of-sequence restart marker");
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (uint32_t c = 0; c < f.ncomp; ++c) {
                const Huff &dc = f.dc[f.comp[c].td], &ac = f.ac[f.comp[c].ta];
                const uint32_t h = f.comp_h(c), v = f.comp_v(c);
                for (uint32_t by = 0; by < v; ++by) {
                    for (uint32_t bx = 0; bx < h; ++bx) {
                        const uint64_t b = (static_cast<uint64_t>(my) * v + by) * f.blocks_w(c) + (static_cast<uint64_t>(mx) * h + bx);
                        int16_t *out = plane[c] + pixo_jdec::coef_index(b, 0); // + (natural >> 3) * 512 + (natural & 7)
                        const int t = decode_symbol(br, dc);
                        if (t < 0 || t > 15) return refuse(INVALID, msg, br.overran() ? "entropy-coded segment ends early" : "Huffman code not in the table");
                        if (t) pred[c] += static_cast<uint32_t>(extend(br.take(t), t));
                        out[0] = static_cast<int16_t>(pred[c]);
                        for (int k = 1; k < 64;) {
                            const int s = decode_symbol(br, ac);
                            if (s < 0) return refuse(INVALID, msg, br.overran() ? "entropy-coded segment ends early" : "Huffman code not in the table");
                            const int run = s >> 4, size = s & 15;
                            if (size == 0) {
                                if (run != 15) break; // end of block
                                k += 16;
                                if (k > 64) return refuse(INVALID, msg, "coefficient index past 63");
                                continue;
                            }
                            k += run;
                            if (k > 63) return refuse(INVALID, msg, "coefficient index past 63");
                            const uint32_t natural = kZigzag[k];
                            out[(natural >> 3) * 512 + (natural & 7)] = static_cast<int16_t>(extend(br.take(size), size));
                            ++k;
                        }
                        if (br.overran()) return refuse(INVALID, msg, "entropy-coded segment ends early");
                    }
                }
            }
        }
    }
    return OK;
}

} // namespace pixo_jdec_host
